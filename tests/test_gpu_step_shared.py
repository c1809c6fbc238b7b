"""The native Engine and the autograd op issue ONE launch sequence (csrc/runtime/step.cpp), so one
Engine step and one ``ntxent_loss(h).backward()`` on the same input return the same loss and the
same gradient, bit for bit, on every branch of that sequence. Each case first confirms with
``step_plan`` (the decisions both callers resolve) that its shape really takes the branch it is
here for. Shapes: the smallest that reach each branch.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 0.07


def _h(rows, dim, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, dim, generator=g).to("cuda", dtype)


def _plan(ext, rows, dim, dtype, compute, keep):
    name = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}[dtype]
    comp = compute if compute != "auto" else ("fp32" if dtype == torch.float32 else "fp16")
    return ext.step_plan(rows, dim, name, comp, keep, ext.device_info(0)["num_cus"])


def _both(ext, rows, dim, dtype=torch.bfloat16, compute="auto", keep=True):
    """(engine loss, engine dh, op loss, op grad) of one step each on the same seeded input."""
    import ntxent_amd

    h = _h(rows, dim, rows + dim, dtype)
    name = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}[dtype]
    eng = ext.NativeEngine(rows, dim, T, name, compute, keep_cos=keep)
    loss, dh = eng.step(h)
    x = h.clone().requires_grad_(True)
    ref = ntxent_amd.ntxent_loss(x, T, compute=compute, keep_logits=keep)
    ref.backward()
    torch.cuda.synchronize()
    return loss, dh, ref.detach(), x.grad


def _assert_same(loss, dh, ref, grad):
    assert torch.isfinite(ref).item() and torch.isfinite(grad).all()
    assert loss.item() == ref.item(), (loss.item(), ref.item())
    assert torch.equal(dh, grad), f"max diff {(dh.float() - grad.float()).abs().max().item()}"


# (rows, dim, dtype, the plan fields that name the branch)
CASES = [
    pytest.param(256, 64, torch.bfloat16, dict(small=True, small_fwd_fused=True), id="small-fused-prologue"),
    pytest.param(2048, 128, torch.bfloat16, dict(small=True, small_fwd_fused=False), id="small-with-prep"),
    pytest.param(8192, 256, torch.bfloat16, dict(small=False, raw=True, fuse=True, half_c=True, dfold=True),
                 id="raw-diag-remainder"),
    pytest.param(4096, 512, torch.bfloat16, dict(small=False, raw=True, fuse=True), id="raw-no-remainder"),
    pytest.param(2500, 320, torch.bfloat16, dict(small=False, raw=False, fuse=True), id="unit-rows-fused-norm"),
    pytest.param(2500, 300, torch.bfloat16, dict(small=False, raw=False, fuse=False), id="unfused-norm"),
    pytest.param(2304, 192, torch.float32, dict(small=False, raw=False, fuse=False, bwd="fp32"), id="fp32-exact"),
]


@pytest.mark.parametrize("rows,dim,dtype,branch", CASES)
def test_engine_step_bitwise_equals_autograd_op(ext, rows, dim, dtype, branch):
    plan = _plan(ext, rows, dim, dtype, "auto", True)
    assert {k: plan[k] for k in branch} == branch
    # the diagonal remainder of the forward launch: 16 tiles at (8192, 256) on 256 CUs, none at (4096, 512)
    cus = ext.device_info(0)["num_cus"]
    rem = ext.fwd_diag_remainder(plan["n_fwd"], ext.geometry(rows, dim)["dim_k"] * 2 // ext.K_STEP_BYTES, cus,
                                 ext.geometry(rows, dim)["row_tiles"])
    if (rows, dim) == (8192, 256) and cus == 256:
        assert rem == 16
    if (rows, dim) == (4096, 512):
        assert rem == 0
    _assert_same(*_both(ext, rows, dim, dtype))


@pytest.mark.parametrize("q8", [True, False], ids=["fp8-backward", "fp16-backward"])
def test_engine_step_bitwise_equals_autograd_op_fp8(ext, q8):
    rows, dim = 4096, 256
    old = ext.fp8_backward_enabled()
    try:
        ext.set_fp8_backward(q8)
        plan = _plan(ext, rows, dim, torch.bfloat16, "fp8", True)
        assert plan["f8"] and plan["q8"] == q8 and not plan["fuse"] and not plan["small"]
        out = _both(ext, rows, dim, compute="fp8")
    finally:
        ext.set_fp8_backward(old)
    _assert_same(*out)


def test_engine_step_bitwise_equals_autograd_op_recompute(ext):
    rows, dim = 4096, 256
    plan = _plan(ext, rows, dim, torch.bfloat16, "auto", False)
    assert not plan["keep_cos"] and not plan["raw"] and not plan["half_c"] and plan["fuse"] and not plan["small"]
    _assert_same(*_both(ext, rows, dim, keep=False))
