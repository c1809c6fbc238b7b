"""Cross-view InfoNCE kernels (csrc/kernels/xview_kernels.hip) and the public op on an MI355X.

Parity bound (group 1): 2 x max(the project's table for the same arithmetic, the error the existing
ntxent_loss shows against its own oracle on the same input and compute in the same run). Largest
errors of info_nce_loss measured on MI355X over the shapes below (loss rel / dh rel to max|g| / dtau
rel): fp32 6.6e-10 / 5.1e-6 / 6.2e-7, fp16 3.4e-8 / 1.1e-3 / 3.0e-5, bf16 4.3e-7 / 6.5e-3 / 3.4e-4
("Cross-view InfoNCE").

The exact cases (group 2) ask for "the fp32 tolerance" in every compute dtype: that is the group-1
bound of the fp32 run, 2 x max(fp32 table value, the error of ntxent_loss with compute="fp32" on the
same input), one bound for all three computes. (A yardstick in the 16-bit compute would be far too
wide: ntxent_loss's 16-bit small path rounds its coefficients to 16 bits once, which on one-hot rows
is the very error the two coefficient planes exist to avoid.)
"""
import functools
import math

import pytest
import torch

import ntxent_amd
from ntxent_amd.ops import reference as R

pytestmark = pytest.mark.gpu

# test_gpu_kernels.TOL and test_gpu_temperature_grad.TOL_TAU: (loss rtol, dh err / max|g|, dtau rtol)
TABLE = {"fp32": (2e-9, 6e-6, 4.5e-7), "fp16": (1.2e-6, 8e-3, 6.1e-4), "bf16": (7e-7, 2.2e-2, 3e-4)}

SHAPES = [(37, 40), (128, 64), (200, 100), (384, 256)]
CASES = ([(n, d, "fp32") for n, d in SHAPES] + [(n, d, c) for n, d in [(200, 100), (384, 256)] for c in ("fp16", "bf16")]
         + [(1024, 512, "fp16")]
         # two tiles per side, the second all but one row padding; d = 160 is an odd number (3) of 16-bit K-steps
         + [(129, 160, "fp32"), (129, 160, "fp16"), (129, 160, "bf16"), (37, 160, "fp16")])


def _inputs(rows, dim, dtype, seed=0, noise=0.3):
    g = torch.Generator().manual_seed(seed)
    n = rows // 2
    base = torch.randn(n, dim, generator=g, dtype=torch.float64)
    v1 = base + noise * torch.randn(n, dim, generator=g, dtype=torch.float64)
    v2 = base + noise * torch.randn(n, dim, generator=g, dtype=torch.float64)
    h64 = torch.cat([v1, v2], 0)
    return h64, h64.to(dtype).cuda()


def _oracle(fn, h_dev, T):
    """(loss, dh, dtau) of `fn` in fp64 on the device tensor cast to double."""
    x = h_dev.detach().double().requires_grad_(True)
    tau = torch.tensor(T, dtype=torch.float64, device=x.device, requires_grad=True)
    gh, gt = torch.autograd.grad((loss := fn(x, tau)), (x, tau))
    return loss.item(), gh, gt.item()


@functools.lru_cache(maxsize=None)
def _case(n, d, T=0.07):
    _, h = _inputs(2 * n, d, torch.float32, seed=n + d)
    return h, _oracle(R.info_nce_loss, h, T), _oracle(R.ntxent_loss, h, T)


def _run(fn, h, temperature, compute, scale=None, **kw):
    x = h.clone().requires_grad_(True)
    loss = fn(x, temperature, compute=compute, **kw)
    (loss if scale is None else scale * loss).backward()
    dtau = temperature.grad if isinstance(temperature, torch.Tensor) and temperature.is_leaf else None
    return loss.detach(), x.grad, dtau


def _tau(T):
    return torch.tensor(T, dtype=torch.float32, device="cuda", requires_grad=True)


def _errors(out, ref):
    loss, dh, dtau = out
    lref, gref, tref = ref
    return (abs(loss.item() - lref) / max(1.0, abs(lref)),
            (dh.double() - gref).abs().max().item() / max(gref.abs().max().item(), 1e-300),
            abs(dtau.item() - tref) / max(abs(tref), 1e-300))


# ---- 1. parity with the fp64 oracle -----------------------------------------------------------
@pytest.mark.parametrize("n,d,compute", CASES)
def test_parity_with_the_oracle(gpu, n, d, compute):
    h, ref_x, ref_n = _case(n, d)
    e_new = _errors(_run(ntxent_amd.info_nce_loss, h, _tau(0.07), compute), ref_x)
    e_old = _errors(_run(ntxent_amd.ntxent_loss, h, _tau(0.07), compute), ref_n)
    bound = tuple(2.0 * max(t, e) for t, e in zip(TABLE[compute], e_old))
    print(f"XVPARITY n={n} d={d} compute={compute} infonce loss/dh/dtau={e_new[0]:.3e}/{e_new[1]:.3e}/{e_new[2]:.3e} "
          f"ntxent={e_old[0]:.3e}/{e_old[1]:.3e}/{e_old[2]:.3e} bound={bound[0]:.3e}/{bound[1]:.3e}/{bound[2]:.3e}")
    assert all(math.isfinite(e) for e in e_new)
    assert e_new[0] <= bound[0] and e_new[1] <= bound[1] and e_new[2] <= bound[2], (e_new, bound)


# ---- 2. exact cases -----------------------------------------------------------------------------
def _fp32_bound(h, T):
    """The fp32 tolerance of group 1 on this input, the same for every compute dtype of the op under
    test: 2 x max(fp32 table value, what ntxent_loss with compute="fp32" shows against its own oracle
    here) for (loss, dh)."""
    e_old = _errors(_run(ntxent_amd.ntxent_loss, h, _tau(T), "fp32"), _oracle(R.ntxent_loss, h, T))
    return 2.0 * max(TABLE["fp32"][0], e_old[0]), 2.0 * max(TABLE["fp32"][1], e_old[1])


@pytest.mark.parametrize("compute", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("n,d", [(37, 40), (200, 100)])
def test_identical_rows(gpu, n, d, compute):
    """Every cosine is 1: the loss is log N (a counted pad column would give log(roundup))."""
    row = torch.randn(d, generator=torch.Generator().manual_seed(1))
    h = row.repeat(2 * n, 1).cuda()
    loss, dh, _ = _run(ntxent_amd.info_nce_loss, h, 0.07, compute)
    lt, _ = _fp32_bound(h, 0.07)
    err = abs(loss.item() - math.log(n)) / math.log(n)
    worst = (dh.abs().max(1).values * h.norm(dim=1)).max().item()
    print(f"XVEXACT identical n={n} d={d} compute={compute} loss_rel_err={err:.3e} bound={lt:.3e} dh*|h|={worst:.3e}")
    assert err <= lt, (loss.item(), math.log(n), lt)
    assert worst <= 1e-6


@pytest.mark.parametrize("compute", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("n", [37, 200])
def test_orthogonal_rows(gpu, n, compute):
    """One-hot rows are exact in every dtype: the same (fp32) tolerance for every compute.

    Measured on MI355X (loss rel / dh rel to max|g|): N = 37: fp32 2.3e-8 / 2.4e-7, fp16 2.3e-8 /
    2.4e-7, bf16 2.3e-8 / 1.9e-6; N = 200: fp32 2.2e-8 / 2.1e-7, fp16 2.2e-8 / 2.1e-7, bf16 2.2e-8 /
    2.8e-6. Every negative's coefficient is the same number here, 2 / (e^2 + N - 1), so a backward
    that rounds its coefficients to 16 bits once shows that rounding undiminished (fp16, N = 37:
    2.8e-4); the coefficient planes (rounded value + scaled residual) and the fp32 dZ slab are what
    meets the fp32 bound in the 16-bit computes."""
    dp = (n + 63) // 64 * 64
    v = 3.0 * torch.eye(n, dp)
    h = torch.cat([v, v], 0).cuda()
    loss, dh, _ = _run(ntxent_amd.info_nce_loss, h, 0.5, compute)
    want = math.log1p((n - 1) * math.exp(-2.0))
    _, gref, _ = _oracle(R.info_nce_loss, h, 0.5)
    lt, gt = _fp32_bound(h, 0.5)
    le = abs(loss.item() - want) / max(1.0, want)
    ge = (dh.double() - gref).abs().max().item() / gref.abs().max().item()
    print(f"XVEXACT orthogonal n={n} compute={compute} loss_rel_err={le:.3e} bound={lt:.3e} dh_rel_err={ge:.3e} bound={gt:.3e}")
    assert le <= lt, (loss.item(), want)
    assert ge <= gt


@pytest.mark.parametrize("compute", ["fp32", "fp16", "bf16"])
def test_single_pair(gpu, compute):
    _, h = _inputs(2, 40, torch.float32, seed=2)
    loss, dh, _ = _run(ntxent_amd.info_nce_loss, h, 0.07, compute)
    assert loss.item() == 0.0 and dh.abs().max().item() <= 1e-6


# ---- 3. stability ----------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-5, 1.0, 1e5])
@pytest.mark.parametrize("T", [0.01, 0.07, 1.0])
def test_numerical_stability_grid(gpu, scale, T):
    g = torch.Generator().manual_seed(11)
    z = (torch.nn.functional.normalize(torch.randn(256, 256, generator=g), dim=1) * scale).cuda()
    loss, gr, _ = _run(ntxent_amd.info_nce_loss, z, T, "fp32")
    assert torch.isfinite(loss) and torch.isfinite(gr).all()
    lref, gref, _ = _oracle(R.info_nce_loss, z, T)
    assert abs(loss.item() - lref) <= 1e-4 * max(1.0, abs(lref))
    assert (gr.double() - gref).abs().max() <= 1e-3 * gref.abs().max() + 1e-12


def test_identical_views_at_low_temperature(gpu):
    """h2 = h1 at tau = 0.01: P_ip -> 1, where 1 - P would cancel."""
    _, h = _inputs(256, 64, torch.float32, seed=4)
    h = torch.cat([h[:128], h[:128]], 0)
    out = _run(ntxent_amd.info_nce_loss, h, _tau(0.01), "fp32")
    assert torch.isfinite(out[0]) and torch.isfinite(out[1]).all() and torch.isfinite(out[2])
    e_new = _errors(out, _oracle(R.info_nce_loss, h, 0.01))
    e_old = _errors(_run(ntxent_amd.ntxent_loss, h, _tau(0.01), "fp32"), _oracle(R.ntxent_loss, h, 0.01))
    print(f"XVSHARP infonce={e_new} ntxent={e_old}")
    assert all(e <= 2.0 * max(t, o) for e, t, o in zip(e_new, TABLE["fp32"], e_old)), (e_new, e_old)


def test_zero_row_is_finite(gpu):
    _, h = _inputs(128, 64, torch.float32)
    h[3] = 0
    loss, g, _ = _run(ntxent_amd.info_nce_loss, h, 0.07, "fp32")
    assert torch.isfinite(loss) and torch.isfinite(g).all()


# ---- 4. autograd behaviour -----------------------------------------------------------------------
def test_grad_out_scaling(gpu):
    h, _, _ = _case(200, 100)
    _, g1, t1 = _run(ntxent_amd.info_nce_loss, h, _tau(0.07), "fp32")
    _, g35, t35 = _run(ntxent_amd.info_nce_loss, h, _tau(0.07), "fp32", scale=3.5)
    assert (g35 - 3.5 * g1).abs().max().item() <= 2e-7 * (3.5 * g1).abs().max().item()
    assert abs(t35.item() - 3.5 * t1.item()) <= 2e-7 * abs(3.5 * t1.item())


def test_two_leaves_each_get_their_half(gpu):
    h, _, _ = _case(200, 100)
    _, g, _ = _run(ntxent_amd.info_nce_loss, h, 0.07, "fp32")
    a, b = h[:200].clone().requires_grad_(True), h[200:].clone().requires_grad_(True)
    ntxent_amd.info_nce_loss(a, 0.07, z2=b, compute="fp32").backward()
    assert torch.equal(a.grad, g[:200]) and torch.equal(b.grad, g[200:])
    ntxent_amd.InfoNCELoss(0.07, compute="fp32")(a, b).backward()  # accumulates the same again
    assert torch.equal(a.grad, 2 * g[:200])


@pytest.mark.parametrize("compute", ["fp32", "fp16", "fp8"])
def test_tensor_temperature_is_bitwise_the_float(gpu, compute):
    h, _, _ = _case(200, 100)
    lf, gf, _ = _run(ntxent_amd.info_nce_loss, h, 0.07, compute)
    tau = _tau(0.07)
    lt, gt, dt = _run(ntxent_amd.info_nce_loss, h, tau, compute)
    assert torch.equal(lf, lt) and torch.equal(gf, gt)
    assert dt.shape == tau.shape and dt.dtype == tau.dtype and dt.device == tau.device
    if compute == "fp8":  # computes in fp16
        l16, g16, _ = _run(ntxent_amd.info_nce_loss, h, 0.07, "fp16")
        assert torch.equal(lf, l16) and torch.equal(gf, g16)


def test_log_scale_temperature(gpu):
    h, _, _ = _case(200, 100)
    _, _, dt = _run(ntxent_amd.info_nce_loss, h, _tau(0.07), "fp32")
    ls = torch.tensor(math.log(0.07), dtype=torch.float32, device="cuda", requires_grad=True)
    x = h.clone().requires_grad_(True)
    ntxent_amd.info_nce_loss(x, ls.exp(), compute="fp32").backward()
    tv = math.exp(math.log(0.07))
    assert abs(ls.grad.item() - tv * dt.item()) <= 1e-5 * abs(tv * dt.item())
    m = ntxent_amd.InfoNCELoss(0.07, compute="fp32", learnable_temperature=True).cuda()
    m(h).backward()
    assert abs(m.log_temperature.grad.item() - ls.grad.item()) <= 1e-5 * abs(ls.grad.item())


def test_retain_graph_twice(gpu):
    h, _, _ = _case(200, 100)
    x = h.clone().requires_grad_(True)
    tau = _tau(0.07)
    loss = ntxent_amd.info_nce_loss(x, tau, compute="fp16")
    g1 = torch.autograd.grad(loss, (x, tau), retain_graph=True)
    g2 = torch.autograd.grad(loss, (x, tau))
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])


# ---- 5. determinism and isolation -----------------------------------------------------------------
@pytest.mark.parametrize("n,d,compute", [(384, 256, "bf16"), (1024, 512, "fp16")])
def test_deterministic(gpu, n, d, compute):
    h, _, _ = _case(n, d)
    a = _run(ntxent_amd.info_nce_loss, h, _tau(0.07), compute)
    b = _run(ntxent_amd.info_nce_loss, h, _tau(0.07), compute)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_does_not_disturb_ntxent(gpu):
    """An info_nce_loss forward + backward between ntxent_loss's forward and backward changes neither."""
    _, h = _inputs(1024, 256, torch.bfloat16, seed=9)
    alone = _run(ntxent_amd.info_nce_loss, h, 0.1, "auto")

    def run(between):
        x = h.clone().requires_grad_(True)
        loss = ntxent_amd.ntxent_loss(x, 0.1)
        got = _run(ntxent_amd.info_nce_loss, h, 0.1, "auto") if between else None
        loss.backward()
        return loss.detach().clone(), x.grad.clone(), got

    l0, g0, _ = run(False)
    l1, g1, got = run(True)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    assert torch.equal(got[0], alone[0]) and torch.equal(got[1], alone[1])


def test_side_stream(gpu):
    h, _, _ = _case(200, 100)
    want = _run(ntxent_amd.info_nce_loss, h, _tau(0.07), "fp16")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = _run(ntxent_amd.info_nce_loss, h, _tau(0.07), "fp16")
    s.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_graph_capture_replay(gpu):
    """No host sync, no blocking allocation: forward + backward capture into a CUDAGraph, and a replay
    on new contents of the captured input gives what the eager run on them gave."""
    n, d = 200, 100
    h0, _, _ = _case(n, d)
    _, h1 = _inputs(2 * n, d, torch.float32, seed=77)
    want0 = _run(ntxent_amd.info_nce_loss, h0, 0.07, "fp16")  # (the plan exists from here on)
    want1 = _run(ntxent_amd.info_nce_loss, h1, 0.07, "fp16")
    torch.cuda.synchronize()
    x = h0.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on the side stream, as torch asks before a capture
        (g,) = torch.autograd.grad(ntxent_amd.info_nce_loss(x, 0.07, compute="fp16"), x)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = ntxent_amd.info_nce_loss(x, 0.07, compute="fp16")
        (g,) = torch.autograd.grad(loss, x)
    for src, want in ((h0, want0), (h1, want1)):
        with torch.no_grad():
            x.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), want[0]) and torch.equal(g, want[1])
    assert not torch.equal(want0[0], want1[0])


def test_prep_is_bitwise_repeatable(ext, gpu):
    """The backward runs the row prologue again instead of keeping the forward's unit rows, and forms
    the coefficients from the second copy with the lse2 / cpos of the first: they must be the same
    bits (ntxent_torch.cpp, xview_backward_impl)."""
    h, _, _ = _case(200, 100)
    for x, compute in ((h, "fp32"), (h, "fp16"), (h.bfloat16(), "bf16")):
        plan = ext.get_plan(400, 100, 1, 0, 0.07, compute, gpu.index)
        a = [t.clone() for t in ext.prep(x, plan)[:3]]  # zq, inv, ypos
        b = ext.prep(x, plan)[:3]
        assert all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(a, b)), compute


# ---- 6. memory ---------------------------------------------------------------------------------
def test_memory_peak_within_the_issues_bound(gpu):
    """The peak over forward + backward stays below the issue's bound: the input rows, zq and its
    transpose, dh, one 16-bit N x N buffer and 1 MiB.

    What the bound does and does not show here: 16-bit plans hold the coefficient block as two 16-bit
    planes, 4 N_pad^2 bytes, which is as large as one fp32 square would be (twice the one 16-bit
    buffer the issue had in mind; the orthogonal exact case needs the second plane). No fp32 N x N
    *logit or probability* data exists, but the test passes because the backward releases buffers
    stage by stage (the unit rows before the fp32 dZ slab, coefficients and transposes before dh),
    so the planes never coexist with everything else: measured peak 10 MiB against the 11 MiB bound.
    A third plane, or holding zq across the backward, would break it."""
    n, d = 1024, 512
    _, h = _inputs(2 * n, d, torch.float16, seed=n + d)
    _run(ntxent_amd.info_nce_loss, h, 0.07, "fp16")  # plan, scratch
    x = h.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = ntxent_amd.info_nce_loss(x, 0.07, compute="fp16")
    loss.backward()
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    bound = 2 * n * d * (2 + 2 * 2 + 2) + n * n * 2 + (1 << 20)
    print(f"XVMEM delta={delta} bound={bound}")
    assert delta < bound, (delta, bound)


# ---- 7. trainer -----------------------------------------------------------------------------------
def test_trainer_on_the_gpu(gpu):
    from ntxent_amd.models.trainer import SimCLRTrainer, TrainConfig

    cfg = TrainConfig(steps=2, batch=32, image_size=8, encoder="mlp", proj_hidden=32, proj_out=16, warmup_steps=1,
                      log_every=0, metrics_every=2, loss="infonce", learnable_temperature=True)
    hist = SimCLRTrainer(cfg, device=gpu).fit()
    assert len(hist) == 2 and all(math.isfinite(r["loss"]) for r in hist)
    assert "top1" in hist[0] and "top1" not in hist[1]
    assert abs(hist[-1]["temperature"] - 0.5) > 1e-7
