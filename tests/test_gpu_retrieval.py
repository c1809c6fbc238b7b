"""Cross-view retrieval-rank kernels (csrc/kernels/xview_rank_kernels.hip) and their public API on
the GPU.

As in test_gpu_metrics.py a rank is an integer count of comparisons, so it is bracketed between the
fp64 oracle's counts of ``cos > t + delta`` and ``cos > t - delta`` on the very rows the kernel
read, after checking on the oracle alone that the bracket is tight for 90 % of the rows; the planted
case pins both directions, the masks and the tie-break exactly.
"""
import functools

import pytest
import torch

import ntxent_amd
from ntxent_amd.ops import reference as R
from test_retrieval_cpu import check_planted, planted

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
# one partial tile | two tiles per side, the second one row deep, view 2 off tile alignment, three
# 16-bit K-steps | exact tiles | 3 x 3 tiles: off-diagonal tiles in both orientations
SHAPES = [(37, 40), (129, 160), (256, 64), (300, 100)]
DTYPES = ["fp32", "fp16", "bf16"]


@functools.lru_cache(maxsize=None)
def _views(n, d, dt):
    """test_gpu_metrics.py's data: h2 = s * h1 + noise, s ~ U[0, 1.5] per row, pair 0 negated."""
    g = torch.Generator().manual_seed(0)
    h1 = torch.randn(n, d, generator=g)
    s = 1.5 * torch.rand(n, 1, generator=g)
    s[0] = -s[0]
    h2 = s * h1 + torch.randn(n, d, generator=g)
    return torch.cat([h1, h2], 0).to(DT[dt])


def _stage(ext, gpu, h, dt):
    plan = ext.get_plan(h.shape[0], h.shape[1], 1, 0, 0.07, dt, gpu.index)
    zq = ext.prep(h, plan)[0]
    return ext.xview_rank(zq, plan), zq.view(plan.rows_pad, plan.ld_k)[: h.shape[0], : h.shape[1]]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_stage_op_within_the_fp64_bracket(ext, gpu, n, d, dt):
    """_C.xview_rank on prep's unit rows against fp64 on those very rows: only fp32 accumulation
    separates the two (16-bit products are exact in fp32), so delta = d * 2^-22."""
    (rank, pos, hard, index), rows = _stage(ext, gpu, _views(n, d, dt).to(gpu), dt)
    assert [t.dtype for t in (rank, pos, hard, index)] == [torch.int32, torch.float32, torch.float32, torch.int32]
    assert rank.shape == pos.shape == hard.shape == index.shape == (2 * n,)
    delta = d * 2.0 ** -22
    z = rows.cpu().double()
    lo, hi = R.retrieval_rank_bounds(z, delta)
    S = z[:n] @ z[n:].t()
    t = S.diagonal().repeat(2)
    both = torch.cat([S, S.t()], 0)
    both[torch.arange(2 * n), torch.arange(n).repeat(2)] = float("-inf")  # the row's own pair
    hmax = both.max(1).values
    loose = (lo != hi).float().mean().item()
    print(f"stage {n}x{d} {dt}: rows with lo != hi {100 * loose:.2f} %")
    assert loose <= 0.10, "the bracket must be tight for 90 % of the rows, or it could hide a failure"
    rank, pos, hard, index = rank.cpu().long(), pos.cpu().double(), hard.cpu().double(), index.cpu().long()
    bad = ((rank < lo) | (rank > hi)).nonzero().flatten()
    at_index = both.gather(1, index.clamp(0, n - 1).unsqueeze(1)).squeeze(1)
    print(f"  rank {int(rank.min())}..{int(rank.max())}, outside the bracket {bad.numel()}, directions differ in "
          f"{int((rank[:n] != rank[n:]).sum())} pairs, max |pos - t| {float((pos - t).abs().max()):.3e}, |hard - oracle| "
          f"{float((hard - hmax).abs().max()):.3e}, oracle gap at index {float((hmax - at_index).max()):.3e}, delta {delta:.3e}")
    assert bad.numel() == 0, (bad[:8].tolist(), rank[bad[:8]].tolist(), lo[bad[:8]].tolist(), hi[bad[:8]].tolist())
    assert (pos - t).abs().max().item() <= delta and torch.equal(pos[:n], pos[n:])
    assert (hard - hmax).abs().max().item() <= delta
    assert ((index >= 0) & (index < n)).all() and (index != torch.arange(n).repeat(2)).all()
    assert (hmax - at_index).max().item() <= delta
    assert int(rank.min()) == 0 and int(rank.max()) == n - 1  # the data spans the ranks ...
    assert not torch.equal(rank[:n], rank[n:])  # ... and the two directions differ


@pytest.mark.parametrize("dt", DTYPES)
def test_planted_case_is_exact(gpu, dt):
    """Both directions, the pad and other-view masks, a candidate in the other tile and the
    lowest-index tie-break, on cosines that every dtype holds exactly apart."""
    rank, pos, hard, index = ntxent_amd.retrieval_rank(planted(dtype=DT[dt]).to(gpu), compute=dt)
    check_planted(rank, index)
    assert (hard[5] == 0) and (hard[130 + 5] == 0) and abs(float(hard[130]) - 4 / 30 ** 0.5) < 1e-2


@pytest.mark.parametrize("dt", DTYPES)
def test_single_pair(gpu, dt):
    rank, pos, hard, index = ntxent_amd.retrieval_rank(_views(1, 40, dt).to(gpu), compute=dt)
    assert rank.tolist() == [0, 0] and index.tolist() == [-1, -1]
    assert (hard == float("-inf")).all() and pos[0] == pos[1] and torch.isfinite(pos).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_public_op_is_the_stage_op_and_repeats(ext, gpu, dt):
    n, d = 300, 100
    h = _views(n, d, dt).to(gpu)
    want, _ = _stage(ext, gpu, h, dt)
    for _ in range(2):
        got = ntxent_amd.retrieval_rank(h[:n], z2=h[n:], compute=dt)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want))
    m = ntxent_amd.retrieval_metrics(h, compute=dt)
    assert all(v.dim() == 0 and v.device == h.device for v in m.values())
    rank = want[0]
    for k in (1, 5, 10):
        one, two = float((rank[:n] < k).float().mean()), float((rank[n:] < k).float().mean())
        assert (float(m[f"top{k}_1to2"]), float(m[f"top{k}_2to1"])) == (one, two)
        assert abs(float(m[f"top{k}"]) - (one + two) / 2) < 1e-6
    assert int(m["negatives"]) == n - 1
