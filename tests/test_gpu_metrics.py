"""Positive-rank kernel (csrc/kernels/rank_kernels.hip) and the contrastive-metrics API on the GPU.

The rank is an integer count of comparisons ``cos_ij > t_i``; a cosine the kernel computes within
``delta / 2`` of the oracle's can flip a comparison only where the oracle's margin is below
``delta``. The tests therefore bracket the rank between the oracle's counts of ``cos > t + delta``
and ``cos > t - delta`` (``reference.positive_rank_bounds``), after checking on the oracle alone
that the bracket is tight (``lo == hi``) for at least 90 % of the rows, and pin the hand-built
cases (identical views, opposite views, a single pair) exactly.
"""
import functools

import pytest
import torch

import ntxent_amd
from ntxent_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
# (N, d, input dtype): rows that are no tile multiple, d that is no multiple of 64, positive pairs
# that straddle tiles, several tiles per side, all three MFMA types
SHAPES = [(37, 40, "fp32"), (256, 64, "fp16"), (256, 64, "bf16"), (513, 100, "fp16"), (1024, 256, "bf16"),
          (1024, 256, "fp32"),
          # d = 160: an odd number (3) of 16-bit K-steps, on diagonal and off-diagonal tiles and on a single tile
          (129, 160, "fp16"), (129, 160, "bf16"), (37, 160, "fp16")]
SEED = 0


@functools.lru_cache(maxsize=None)
def _views(n, d, dt, seed=SEED):
    """h1 random, h2 = s * h1 + noise with one s ~ U[0, 1.5] per row: the ranks spread from 0 to
    about 2N. Pair 0 takes -s: at large d and small n the draw alone leaves every positive in front
    (37 x 160: all ranks 0), and this pair then still ranks near last. Returned in the input dtype on
    the CPU; shared by every test of the shape."""
    g = torch.Generator().manual_seed(seed)
    h1 = torch.randn(n, d, generator=g)
    s = 1.5 * torch.rand(n, 1, generator=g)
    s[0] = -s[0]
    h2 = s * h1 + torch.randn(n, d, generator=g)
    return torch.cat([h1, h2], 0).to(DT[dt])


def _oracle(z_unit, delta):
    """fp64 (lo, hi, t, hard) of unit rows, computed once per call site (the callers cache)."""
    z = z_unit.double()
    lo, hi = R.positive_rank_bounds(z, delta)
    rows = z.shape[0]
    cos = z @ z.t()
    pos = R.positive_index(rows)
    t = cos[torch.arange(rows), pos]
    masked = cos.clone()
    masked[torch.arange(rows), torch.arange(rows)] = float("-inf")
    masked[torch.arange(rows), pos] = float("-inf")
    return lo, hi, t, masked.max(1).values


@functools.lru_cache(maxsize=None)
def _public_oracle(n, d, dt, delta):
    z, _ = R.normalize(_views(n, d, dt).double())
    return _oracle(z, delta)


def _compute_delta(comp, d):
    # fp16: twice the Cauchy-Schwarz bound 2 * 2^-11 for unit rows rounded to fp16; bf16 likewise
    # with 2^-8; fp32: fp32 accumulation error d * 2^-24 on unit rows, times four
    return {"fp16": 2.0 ** -9, "bf16": 2.0 ** -6, "fp32": d * 2.0 ** -22}[comp]


@pytest.mark.parametrize("n,d,dt", SHAPES)
def test_stage_rank_within_the_fp64_bracket(ext, gpu, n, d, dt):
    """_C.pos_rank on prep's unit rows against fp64 on those very rows: only fp32 accumulation
    separates the two (fp16 / bf16 products are exact in fp32), so delta = d * 2^-22."""
    h = _views(n, d, dt).to(gpu)
    plan = ext.get_plan(2 * n, d, 1, 0, 0.07, dt, gpu.index)
    zq = ext.prep(h, plan)[0]
    rank, pos, hard = ext.pos_rank(zq, plan)
    assert rank.dtype == torch.int32 and pos.dtype == torch.float32 and hard.dtype == torch.float32
    assert rank.shape == pos.shape == hard.shape == (2 * n,)
    delta = d * 2.0 ** -22
    lo, hi, t, hmax = _oracle(zq.view(plan.rows_pad, plan.ld_k)[: 2 * n, :d].cpu(), delta)
    loose = (lo != hi).float().mean().item()
    print(f"stage {n}x{d} {dt}: rows with lo != hi {100 * loose:.2f} %")
    assert loose <= 0.10, "the bracket must be tight for 90 % of the rows, or it could hide a failure"
    rank, pos, hard = rank.cpu().long(), pos.cpu().double(), hard.cpu().double()
    bad = ((rank < lo) | (rank > hi)).nonzero().flatten()
    print(f"  rank range {int(rank.min())}..{int(rank.max())}, outside the bracket: {bad.numel()} rows, "
          f"max |pos - t| {float((pos - t).abs().max()):.3e}, max |hard - oracle| {float((hard - hmax).abs().max()):.3e}, "
          f"delta {delta:.3e}")
    assert bad.numel() == 0, (bad[:8].tolist(), rank[bad[:8]].tolist(), lo[bad[:8]].tolist(), hi[bad[:8]].tolist())
    assert (pos - t).abs().max().item() <= delta
    assert (hard - hmax).abs().max().item() <= delta
    assert int(rank.min()) == 0 and int(rank.max()) > n // 2  # the data exercises both ends


@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("n,d", [(37, 40), (256, 64)])
def test_exact_cases(gpu, n, d, dt):
    """Opposite views: every negative beats the positive (pad rows or columns that were counted, or
    real ones that were dropped, would show); identical views: none does."""
    h1 = _views(n, d, dt)[:n].to(gpu)
    rank, pos, _ = ntxent_amd.positive_rank(torch.cat([h1, -h1], 0), compute=dt)
    assert torch.equal(rank.cpu(), torch.full((2 * n,), 2 * n - 2, dtype=torch.int32)), rank.unique().tolist()
    assert (pos < -0.98).all()
    rank, pos, hard = ntxent_amd.positive_rank(h1, z2=h1.clone(), compute=dt)
    assert torch.equal(rank.cpu(), torch.zeros(2 * n, dtype=torch.int32)), rank.unique().tolist()
    assert (pos > 0.98).all() and (hard < pos).all()


@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
def test_single_pair(gpu, dt):
    h = _views(1, 40, dt).to(gpu)
    rank, pos, hard = ntxent_amd.positive_rank(h, compute=dt)
    assert rank.tolist() == [0, 0]
    assert torch.isinf(hard).all() and (hard < 0).all()
    assert pos[0] == pos[1] and torch.isfinite(pos).all()
    m = ntxent_amd.contrastive_metrics(h, compute=dt)
    assert float(m["top1"]) == 1.0 and int(m["negatives"]) == 0


@pytest.mark.parametrize("n,d,dt", SHAPES)
def test_public_op_within_the_compute_dtype_bracket(gpu, n, d, dt):
    """ntxent_amd.positive_rank / contrastive_metrics on h against the fp64 oracle on h: the unit
    rows are rounded to the compute dtype, so the bracket is that dtype's."""
    delta = _compute_delta(dt, d)
    lo, hi, t, hmax = _public_oracle(n, d, dt, delta)
    h = _views(n, d, dt).to(gpu)
    rank, pos, hard = ntxent_amd.positive_rank(h, compute=dt)
    rank, pos, hard = rank.cpu().long(), pos.cpu().double(), hard.cpu().double()
    print(f"public {n}x{d} {dt}: outside the bracket {int(((rank < lo) | (rank > hi)).sum())} rows, max |pos - t| "
          f"{float((pos - t).abs().max()):.3e}, max |hard - oracle| {float((hard - hmax).abs().max()):.3e}, delta {delta:.3e}")
    assert ((lo <= rank) & (rank <= hi)).all()
    assert (pos - t).abs().max().item() <= delta and (hard - hmax).abs().max().item() <= delta
    m = ntxent_amd.contrastive_metrics(h, compute=dt)
    assert all(v.dim() == 0 and v.device == h.device for v in m.values())
    for k in (1, 5):
        got = float(m[f"top{k}"])
        assert (hi < k).float().mean().item() - 1e-6 <= got <= (lo < k).float().mean().item() + 1e-6, (k, got)
    assert lo.float().mean().item() - 1e-3 <= float(m["mean_rank"]) <= hi.float().mean().item() + 1e-3
    assert int(m["negatives"]) == 2 * n - 2
    assert abs(float(m["pos_cos"]) - t.mean().item()) <= delta
    assert abs(float(m["hard_neg_cos"]) - hmax.mean().item()) <= delta


def test_auto_compute_follows_the_loss_policy(gpu):
    """fp32 input stays exact fp32; bf16 input computes in fp16; "fp8" computes in fp16."""
    n, d = 256, 64
    h32 = _views(n, d, "fp32").to(gpu)
    assert all(torch.equal(a, b) for a, b in zip(ntxent_amd.positive_rank(h32),
                                                 ntxent_amd.positive_rank(h32, compute="fp32")))
    hb = _views(n, d, "bf16").to(gpu)
    want = ntxent_amd.positive_rank(hb, compute="fp16")
    for comp in ("auto", "fp8"):
        assert all(torch.equal(a, b) for a, b in zip(ntxent_amd.positive_rank(hb, compute=comp), want)), comp
    mp = ntxent_amd.positive_rank(h32, use_mixed_precision=True)
    assert all(torch.equal(a, b) for a, b in zip(mp, ntxent_amd.positive_rank(h32, compute="fp16")))


def test_input_validation_on_the_gpu(ext, gpu):
    with pytest.raises(ValueError):
        ntxent_amd.positive_rank(torch.randn(7, 8, device=gpu))
    with pytest.raises((ValueError, RuntimeError)):
        ext.positive_rank(torch.randn(7, 8, device=gpu), "auto", False)
    with pytest.raises((ValueError, RuntimeError)):
        ext.positive_rank(torch.randn(8, device=gpu), "auto", False)
    with pytest.raises((ValueError, RuntimeError)):
        ext.positive_rank(torch.randn(8, 8), "auto", False)


@pytest.mark.parametrize("n,d,dt", [(513, 100, "fp16"), (1024, 256, "bf16")])
def test_deterministic(gpu, n, d, dt):
    h = _views(n, d, dt).to(gpu)
    a = ntxent_amd.positive_rank(h, compute=dt)
    b = ntxent_amd.positive_rank(h, compute=dt)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_does_not_disturb_the_loss(gpu):
    """A positive_rank call between the loss's forward and backward changes neither."""
    h = _views(1024, 256, "bf16").to(gpu)

    def run(between):
        x = h.clone().requires_grad_(True)
        loss = ntxent_amd.ntxent_loss(x, 0.1)
        if between:
            ntxent_amd.positive_rank(x)
        loss.backward()
        return loss.detach().clone(), x.grad.clone()

    l0, g0 = run(False)
    l1, g1 = run(True)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_side_stream(gpu):
    h = _views(513, 100, "fp16").to(gpu)
    want = ntxent_amd.positive_rank(h)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = ntxent_amd.positive_rank(h)
    s.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_graph_capture_replay(gpu):
    """The launch has no host sync and initialises its outputs on the stream: it captures into a
    torch.cuda.CUDAGraph and a replay on new contents of the captured input ranks those."""
    n, d = 513, 100
    h0, h1 = _views(n, d, "fp16").to(gpu), _views(n, d, "fp16", 1).to(gpu)
    want0, want1 = ntxent_amd.positive_rank(h0), ntxent_amd.positive_rank(h1)  # (the plan exists from here on)
    x = h0.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ntxent_amd.positive_rank(x)
    for src, want in ((h0, want0), (h1, want1)):
        x.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(want0[0], want1[0])  # the two inputs do rank differently


def test_native_engine_matches_the_op(gpu):
    from ntxent_amd.parallel.native import NativeNTXent

    n, d = 256, 64
    h = _views(n, d, "bf16").to(gpu)
    eng = NativeNTXent(2 * n, d, 0.07, dtype=torch.bfloat16, compute="bf16")
    nbytes = eng.device_bytes
    loss, dh = eng.step(h)
    eng.forward(h)
    got = eng.positive_rank(h)  # between the engine's forward and backward: neither is disturbed
    dh2 = eng.backward()
    want = ntxent_amd.positive_rank(h, compute="bf16")
    for x, y in zip(got, want):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(dh, dh2) and eng.device_bytes == nbytes


def test_module_and_trainer_on_the_gpu(gpu, tmp_path):
    h = _views(256, 64, "bf16").to(gpu)
    got = ntxent_amd.NTXentLoss(0.2, compute="bf16").metrics(h[:256], h[256:])
    want = ntxent_amd.contrastive_metrics(h, compute="bf16")
    assert all(torch.equal(got[k], want[k]) for k in want)

    from ntxent_amd.models.trainer import SimCLRTrainer, TrainConfig

    cfg = TrainConfig(steps=2, batch=32, image_size=8, encoder="mlp", proj_hidden=32, proj_out=16, warmup_steps=1,
                      log_every=0, metrics_every=2)
    hist = SimCLRTrainer(cfg, device=gpu).fit()
    assert {"top1", "top5", "mean_rank", "pos_cos", "hard_neg_cos", "negatives"} <= set(hist[0])
    assert "top1" not in hist[1] and hist[0]["negatives"] == 62 and 0.0 <= hist[0]["top1"] <= hist[0]["top5"] <= 1.0
