"""Temperature gradient on one GPU (run on an MI355X): d loss / d tau from the autograd op and the
native Engine against autograd through the fp64 oracle on the CPU, on every backward path
(small, fused dZ epilogue with the dot fold on / off / fallback, unfused fp16 and fp32 slabs, fp8
with both backwards, recompute), and what must not move: loss, dh and the plan cache."""
import functools
import math

import pytest
import torch

from ntxent_amd.ops import reference as R
from test_gpu_kernels import TOL, _inputs

pytestmark = pytest.mark.gpu

# |dtau - ref| / |ref| per compute dtype: 2x the largest error measured over the cases below on
# MI355X (profiles/r7/temperature_grad/parity.log: fp32 2.245e-7 at (512,320); fp16 3.013e-4 at
# (34,100), the next 7.3e-5; bf16 1.455e-4 at (1024,512); the kernels are deterministic, so box to
# box these do not move). fp8 measured 1.519e-2 with either backward: the error of the e4m3
# forward's logits (the fp16 path on the same rows: ~1e-4), so twice it would pass the cap and the
# cap itself is the bound. No value is above the gradient tolerance of the same dtype
# (test_gpu_kernels.TOL: fp32 6e-6, fp16 8e-3, bf16 2.2e-2; fp8 1.6e-2, test_gpu_fp8bwd.py): dtau
# is an average of the per-row dot those gradients already use.
TOL_TAU = {"fp32": 4.5e-7, "fp16": 6.1e-4, "bf16": 3e-4, "fp8": 1.6e-2}
assert TOL_TAU["fp32"] <= TOL["fp32"][1] and TOL_TAU["fp16"] <= TOL["fp16"][1] and TOL_TAU["bf16"] <= TOL["bf16"][1]
assert TOL_TAU["fp8"] <= 1.6e-2

_NAME = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}


@functools.lru_cache(maxsize=None)
def _case(rows, dim, in_dtype, T):
    """(h on the GPU, oracle loss, oracle dh, oracle dtau): the oracle is the input as the device
    sees it, cast to fp64 on the CPU, with a tensor temperature. Computed once per case."""
    _, h = _inputs(rows, dim, in_dtype, seed=rows + dim)
    x = h.detach().double().cpu().requires_grad_(True)
    tau = torch.tensor(T, dtype=torch.float64, requires_grad=True)
    loss = R.ntxent_loss(x, tau)
    gh, gt = torch.autograd.grad(loss, (x, tau))
    return h, loss.item(), gh, gt.item()


def _run(h, temperature, compute, keep=True, scale=None):
    """(loss, dh, dtau or None) of the op; `temperature` a float or a tensor."""
    import ntxent_amd

    x = h.clone().requires_grad_(True)
    loss = ntxent_amd.ntxent_loss(x, temperature, compute=compute, keep_logits=keep)
    (loss if scale is None else scale * loss).backward()
    torch.cuda.synchronize()
    dtau = temperature.grad if isinstance(temperature, torch.Tensor) and temperature.is_leaf else None
    return loss.detach(), x.grad, dtau


def _tau(T, device="cuda", dtype=torch.float32):
    return torch.tensor(T, dtype=dtype, device=device, requires_grad=True)


def _plan(ext, rows, dim, in_dtype, compute, keep=True):
    return ext.step_plan(rows, dim, _NAME[in_dtype], compute, keep, ext.device_info(0)["num_cus"])


def _parity(ext, rows, dim, in_dtype, compute, branch, T=0.07, keep=True, tag=""):
    """dtau against the oracle on the path `branch` names (fields of step_plan, asserted), with loss
    and dh bitwise those of the same temperature passed as a float."""
    plan = _plan(ext, rows, dim, in_dtype, compute, keep)
    for k, v in branch.items():
        assert plan[k] == v, (k, plan)
    h, lref, ghref, dref = _case(rows, dim, in_dtype, T)
    loss_f, dh_f, _ = _run(h, T, compute, keep)
    tau = _tau(T)
    loss, dh, dtau = _run(h, tau, compute, keep)
    assert dtau is not None and dtau.shape == tau.shape and dtau.dtype == tau.dtype and dtau.device == tau.device
    err = abs(dtau.item() - dref) / abs(dref)
    print(f"TAUPARITY rows={rows} dim={dim} in={_NAME[in_dtype]} compute={compute} T={T} keep={keep} {tag} "
          f"branch={branch} dtau={dtau.item():.9e} ref={dref:.9e} rel_err={err:.3e}")
    assert torch.equal(loss, loss_f) and torch.equal(dh, dh_f)  # nothing else moves
    if compute in TOL:  # dh as elsewhere (fp8: bitwise the float run's, which test_gpu_fp8*.py bound)
        gerr = (dh.double().cpu() - ghref).abs().max().item() / ghref.abs().max().item()
        assert gerr <= TOL[compute][1], gerr
    assert math.isfinite(dtau.item()) and err <= TOL_TAU[compute], (err, dtau.item(), dref)
    return dtau.item()


def test_small_fused_prologue(ext):
    _parity(ext, 64, 128, torch.bfloat16, "fp16", {"small": True, "small_fwd_fused": True})


def test_small_odd_rows(ext):
    _parity(ext, 34, 100, torch.float32, "fp16", {"small": True})


def test_small_with_prep_and_splits(ext):
    try:
        a = _parity(ext, 2048, 128, torch.float32, "fp16", {"small": True, "small_fwd_fused": False, "small_splits": 8})
        ext.set_small_splits(1)
        b = _parity(ext, 2048, 128, torch.float32, "fp16", {"small": True, "small_fwd_fused": False, "small_splits": 1},
                    tag="splits=1")
    finally:
        ext.set_small_splits(0)
    assert abs(a - b) <= 1e-5 * abs(a)  # the splits only reorder fp32 partial sums of dZ


def test_fused_dot_fold_on_off_fallback(ext):
    fold, spin = ext.dot_fold_enabled(), ext.dot_fold_spin()
    try:
        ext.set_dot_fold(True)
        on = _parity(ext, 512, 320, torch.float32, "fp16", {"small": False, "fuse": True, "dfold": True}, tag="fold")
        ext.set_dot_fold_spin(0)  # every epilogue takes the fallback sum
        fb = _parity(ext, 512, 320, torch.float32, "fp16", {"small": False, "fuse": True, "dfold": True},
                     tag="fold-fallback")
        ext.set_dot_fold_spin(spin)
        ext.set_dot_fold(False)
        off = _parity(ext, 512, 320, torch.float32, "fp16", {"small": False, "fuse": True, "dfold": False},
                      tag="dot_reduce")
    finally:
        ext.set_dot_fold(fold)
        ext.set_dot_fold_spin(spin)
    assert on == off == fb  # the fold is the reduce launch's arithmetic


def test_fused_recompute(ext):
    _parity(ext, 512, 320, torch.float32, "fp16", {"small": False, "fuse": True, "keep_cos": False}, keep=False)


def test_unfused_fp16_slabs_half_c(ext):
    _parity(ext, 2500, 300, torch.float32, "fp16", {"small": False, "fuse": False, "half_c": True, "bwd": "fp16"})


def test_fp32_slabs(ext):
    _parity(ext, 512, 320, torch.float32, "fp32", {"small": False, "fuse": False, "bwd": "fp32"})


@pytest.mark.parametrize("fp8_bwd", [True, False])
def test_fp8_both_backwards(ext, fp8_bwd):
    old = ext.fp8_backward_enabled()
    try:
        ext.set_fp8_backward(fp8_bwd)
        _parity(ext, 1024, 512, torch.bfloat16, "fp8", {"small": False, "f8": True, "q8": fp8_bwd, "fuse": False},
                tag=f"fp8_bwd={fp8_bwd}")
    finally:
        ext.set_fp8_backward(old)


def test_bf16(ext):
    _parity(ext, 1024, 512, torch.float32, "bf16", {"small": False, "fuse": True, "bwd": "bf16"})


def test_dtau_is_deterministic(ext):
    for rows, dim, compute in [(512, 320, "fp16"), (512, 128, "fp16"), (512, 320, "fp32")]:
        h = _case(rows, dim, torch.float32, 0.07)[0]
        a = _run(h, _tau(0.07), compute)[2]
        b = _run(h, _tau(0.07), compute)[2]
        assert torch.equal(a, b), (rows, dim, compute)


@pytest.mark.parametrize("rows,dim,compute,keep,bitwise", [
    (512, 320, "fp32", True, True),    # fp32 keeps and recomputes the same cosines
    (512, 320, "fp32", False, True),
    (512, 320, "fp16", True, False),   # second backward: the coefficient GEMM recomputes the cosines
    (512, 128, "fp16", True, False),   # small path
    (1024, 512, "fp8", True, False),   # fp8 forward, fp16 backward: the second one from the fp16 rows
])
def test_second_backward_retain_graph(ext, rows, dim, compute, keep, bitwise):
    import ntxent_amd

    h, _, _, dref = _case(rows, dim, torch.bfloat16 if compute == "fp8" else torch.float32, 0.07)
    x = h.clone().requires_grad_(True)
    tau = _tau(0.07)
    old = ext.fp8_backward_enabled()
    try:
        # (the e4m3 backward keeps no fp16 Z^T for a second backward, with or without a temperature gradient)
        ext.set_fp8_backward(False)
        loss = ntxent_amd.ntxent_loss(x, tau, compute=compute, keep_logits=keep)
        (_, d1) = torch.autograd.grad(loss, (x, tau), retain_graph=True)
        (_, d2) = torch.autograd.grad(loss, (x, tau))
    finally:
        ext.set_fp8_backward(old)
    e1, e2 = abs(d1.item() - dref) / abs(dref), abs(d2.item() - dref) / abs(dref)
    print(f"TAUPARITY second-backward rows={rows} dim={dim} compute={compute} keep={keep} first={e1:.3e} second={e2:.3e}")
    if bitwise:
        assert torch.equal(d1, d2)
    assert e1 <= TOL_TAU[compute] and e2 <= TOL_TAU[compute], (e1, e2)


def test_grad_out_scales_dtau(ext):
    h, _, _, dref = _case(512, 320, torch.float32, 0.07)
    for compute in ("fp32", "fp16"):
        d1 = _run(h, _tau(0.07), compute)[2].item()
        d35 = _run(h, _tau(0.07), compute, scale=3.5)[2].item()
        assert abs(d35 - 3.5 * d1) <= 2e-7 * abs(3.5 * d1), (d35, d1)  # one fp32 rounding of the product
        assert abs(d35 - 3.5 * dref) <= TOL_TAU[compute] * abs(3.5 * dref)


def test_chain_rule_through_exp(ext):
    import ntxent_amd

    T = 0.2
    h, _, _, dref = _case(512, 320, torch.float32, T)
    log_s = torch.tensor(math.log(T), device="cuda", requires_grad=True)
    x = h.clone().requires_grad_(True)
    ntxent_amd.ntxent_loss(x, log_s.exp(), compute="fp32").backward()
    tau = log_s.detach().exp().item()
    d = _run(h, _tau(tau), "fp32")[2].item()
    assert abs(log_s.grad.item() - d * tau) <= 1e-6 * abs(d * tau)  # exp's backward: one fp32 product
    assert abs(log_s.grad.item() - dref * T) <= 1e-4 * abs(dref * T)  # (tau = fp32 exp(log T), not T)


def test_gradient_lands_on_the_temperatures_device(ext):
    h, _, _, dref = _case(512, 320, torch.float32, 0.07)
    got = {}
    for dev, dt in (("cpu", torch.float32), ("cuda", torch.float32), ("cpu", torch.float64)):
        tau = _tau(0.07, dev, dt)
        d = _run(h, tau, "fp16")[2]
        assert d.device == tau.device and d.dtype == dt and d.shape == tau.shape
        got[(dev, dt)] = d.item()
    assert got[("cpu", torch.float32)] == got[("cuda", torch.float32)]
    # a tensor that does not require grad is a plain value
    x = h.clone().requires_grad_(True)
    import ntxent_amd

    loss = ntxent_amd.ntxent_loss(x, torch.tensor(0.07), compute="fp16")
    assert torch.equal(loss.detach(), _run(h, 0.07, "fp16")[0])


def test_moving_temperature_does_not_leak(ext):
    """200 distinct temperatures at one shape: the tile lists are uploaded once (they do not depend
    on tau) and device memory does not grow."""
    h = _case(512, 320, torch.float32, 0.07)[0]
    mem, uploads = {}, {}
    for i in range(1, 201):
        _run(h, _tau(0.05 + 1e-3 * i), "fp16")
        if i in (2, 200):
            mem[i], uploads[i] = torch.cuda.memory_allocated(), ext.tile_list_uploads()
    assert mem[200] == mem[2], mem
    assert uploads[200] == uploads[2], uploads
    # and a fresh shape uploads its lists exactly once over many temperatures
    n0 = ext.tile_list_uploads()
    plans = [ext.get_plan(768, 72, 1, 0, 0.05 + 1e-3 * i, "fp16", 0) for i in range(100)]
    assert ext.tile_list_uploads() == n0 + 1
    assert all(p.fwd_tiles.data_ptr() == plans[0].fwd_tiles.data_ptr() for p in plans)
    assert abs(plans[7].temperature - 0.057) < 1e-7 and plans[7].rows == 768


# ---- native Engine -----------------------------------------------------------------------
def _engine(rows, dim, T, **kw):
    from ntxent_amd.parallel.native import NativeNTXent

    return NativeNTXent(rows, dim, T, dtype=torch.float32, compute="fp16", **kw)


@pytest.mark.parametrize("rows,dim,small", [(512, 320, False), (512, 128, True)])
def test_engine_temperature_grad(ext, rows, dim, small):
    h, _, _, dref = _case(rows, dim, torch.float32, 0.1)
    eng = _engine(rows, dim, 0.1, temperature_grad=True)
    assert eng.small == small
    loss, dh = eng.step(h)
    dtau = eng.temperature_grad()
    torch.cuda.synchronize()
    op_loss, op_dh, op_dtau = _run(h, _tau(0.1), "fp16")
    err = abs(dtau.item() - dref) / abs(dref)
    print(f"TAUPARITY engine rows={rows} dim={dim} compute=fp16 T=0.1 dtau={dtau.item():.9e} ref={dref:.9e} "
          f"rel_err={err:.3e} op={op_dtau.item():.9e}")
    assert err <= TOL_TAU["fp16"]
    assert abs(dtau.item() - op_dtau.item()) <= TOL_TAU["fp16"] * abs(op_dtau.item())
    # an engine without the option computes the same loss and dh
    plain = _engine(rows, dim, 0.1)
    l0, dh0 = plain.step(h)
    torch.cuda.synchronize()
    assert torch.equal(loss, l0) and torch.equal(dh, dh0)
    with pytest.raises(Exception, match="temperature_grad"):
        plain.temperature_grad()

    # set_temperature: bitwise a fresh engine built at the new value, in the same arena
    nbytes = eng.device_bytes
    eng.set_temperature(0.2)
    assert eng.device_bytes == nbytes and eng.temperature == 0.2
    l2, dh2 = eng.step(h)
    d2 = eng.temperature_grad()
    fresh = _engine(rows, dim, 0.2, temperature_grad=True)
    lf, dhf = fresh.step(h)
    df = fresh.temperature_grad()
    torch.cuda.synchronize()
    assert torch.equal(l2, lf) and torch.equal(dh2, dhf) and torch.equal(d2, df)
    assert not torch.equal(d2, dtau)

    # capture / replay reproduces the eager dtau bitwise; set_temperature drops the graph
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert not eng.captured
        gdh = eng.capture(h)
        assert eng.captured
        lr = eng.replay()
        dr = eng.temperature_grad()
        s.synchronize()
        assert torch.equal(lr, l2) and torch.equal(gdh, dh2) and torch.equal(dr, d2)
        eng.set_temperature(0.1)
        assert not eng.captured
        with pytest.raises(Exception, match="capture"):
            eng.replay()
        l1, dh1 = eng.step(h)
        d1 = eng.temperature_grad()
        s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(l1, loss) and torch.equal(dh1, dh) and torch.equal(d1, dtau)
