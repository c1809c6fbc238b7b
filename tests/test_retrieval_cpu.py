"""Cross-view retrieval ranks without a GPU: the oracles (ops/reference.py), the public functions on
CPU tensors (ops/metrics.py) and the two-tower modules' ``retrieval_metrics``."""
import pytest
import torch

import ntxent_amd
from ntxent_amd.ops import reference as R


def planted(n=130, d=160, dtype=torch.float64):
    """a_i = e_i; b_j = e_j except b_0 = e_0 + 2 e_1 + 3 e_2 + 4 e_3 and b_(n-1) = e_(n-1) + 2 e_0 +
    3 e_1 + 4 e_2: every cosine is 0 or k / sqrt(30), so every comparison is exact in any dtype."""
    a, b = torch.eye(n, d, dtype=dtype), torch.eye(n, d, dtype=dtype)
    b[0, 1:4] = torch.tensor([2.0, 3.0, 4.0], dtype=dtype)
    b[n - 1, 0:3] = torch.tensor([2.0, 3.0, 4.0], dtype=dtype)
    return torch.cat([a, b], 0)


def check_planted(rank, index, n=130):
    """The planted case's exact answer: shared with the GPU test."""
    want = torch.zeros(2 * n, dtype=torch.int32)
    want[n] = want[2 * n - 1] = 3  # b_0 and b_(n-1) see three view-1 rows above their own
    want[0] = 1  # a_0: <a_0, b_(n-1)> = 2 / sqrt(30) beats t_0 = 1 / sqrt(30)
    assert torch.equal(rank.cpu(), want), rank.nonzero().flatten().tolist()
    index = index.cpu()
    # N + 0 -> a_3 (weight 4); N + n - 1 -> a_2, in the other tile; a_0, a_1, a_2 -> b_(n-1) (weights
    # 2, 3, 4 against b_0's 1, 2, 3); a_3 -> b_0; rows whose negatives are all exactly 0 -> candidate
    # 0, the lowest index
    for row, j in ((n, 3), (2 * n - 1, 2), (0, n - 1), (1, n - 1), (2, n - 1), (3, 0), (5, 0), (n + 5, 0)):
        assert int(index[row]) == j, (row, int(index[row]), j)


def _views(n, d, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    h1 = torch.randn(n, d, generator=g, dtype=torch.float64)
    h2 = 1.5 * torch.rand(n, 1, generator=g, dtype=torch.float64) * h1 + torch.randn(n, d, generator=g, dtype=torch.float64)
    return torch.cat([h1, h2], 0).to(dtype)


def test_oracle_planted_case():
    rank, pos, hard, index = R.retrieval_rank(planted())
    assert rank.dtype == torch.int32 and index.dtype == torch.int32 and rank.shape == index.shape == (260,)
    check_planted(rank, index)
    assert torch.equal(pos[:130], pos[130:]) and float(hard[130]) == pytest.approx(4 / 30 ** 0.5)


def test_oracle_identical_opposite_and_single():
    h1 = _views(19, 12)[:19]
    rank, pos, hard, index = R.retrieval_rank(torch.cat([h1, h1], 0))
    assert (rank == 0).all() and torch.allclose(pos, torch.ones_like(pos)) and (hard < 1).all()
    assert (index != torch.arange(19).repeat(2)).all() and (index >= 0).all() and (index < 19).all()
    rank, _, _, _ = R.retrieval_rank(torch.cat([h1, -h1], 0))
    assert (rank == 18).all()
    rank, _, hard, index = R.retrieval_rank(_views(1, 8))
    assert rank.tolist() == [0, 0] and index.tolist() == [-1, -1] and (hard == float("-inf")).all()


def test_bounds_at_zero_are_the_rank_and_bracket_it():
    h = _views(23, 10, seed=3)
    rank = R.retrieval_rank(h)[0]
    z, _ = R.normalize(h)
    assert not torch.equal(rank[:23], rank[23:])  # the two directions differ
    lo0, hi0 = R.retrieval_rank_bounds(z, 0.0)
    assert torch.equal(lo0, hi0) and torch.equal(lo0.to(torch.int32), rank)
    lo, hi = R.retrieval_rank_bounds(z, 0.05)
    assert (lo <= rank).all() and (rank <= hi).all() and (lo < hi).any()


def test_public_functions_on_cpu():
    n = 33
    h = _views(n, 20, seed=2, dtype=torch.float32).requires_grad_(True)
    got, ref = ntxent_amd.retrieval_rank(h), R.retrieval_rank(h.detach())
    assert all(torch.equal(a, b.to(a.dtype)) for a, b in zip(got, ref)) and not any(t.requires_grad for t in got)
    assert [t.dtype for t in got] == [torch.int32, torch.float32, torch.float32, torch.int32]
    m = ntxent_amd.retrieval_metrics(h[:n], z2=h[n:], topk=(1, 5))
    assert set(m) == {f"top{k}{s}" for k in (1, 5) for s in ("", "_1to2", "_2to1")} | {
        "mean_rank", "pos_cos", "hard_neg_cos", "negatives"}
    assert all(v.dim() == 0 and not v.requires_grad for v in m.values())
    assert float(m["top5_1to2"]) == float((got[0][:n] < 5).float().mean())
    assert float(m["top5_2to1"]) == float((got[0][n:] < 5).float().mean())
    assert float(m["top5"]) == pytest.approx((float(m["top5_1to2"]) + float(m["top5_2to1"])) / 2)
    assert int(m["negatives"]) == n - 1 and m["negatives"].dtype == torch.int64


def test_input_validation():
    """The errors of positive_rank."""
    for bad, kw in ((torch.randn(7, 4), {}), (torch.randn(8), {}), (torch.randn(8, 4), {"compute": "int4"})):
        with pytest.raises(ValueError):
            ntxent_amd.retrieval_rank(bad, **kw)
    with pytest.raises(ValueError):
        ntxent_amd.retrieval_metrics(torch.randn(8, 4), topk=(0,))
    with pytest.raises(ValueError):
        R.retrieval_rank(torch.randn(7, 4))


@pytest.mark.parametrize("module", [ntxent_amd.InfoNCELoss, ntxent_amd.SigmoidLoss])
def test_module_retrieval_metrics_match_the_function(module):
    h = _views(12, 8, seed=4, dtype=torch.float32)
    got = module().retrieval_metrics(h[:12], h[12:], topk=(1, 3))
    want = ntxent_amd.retrieval_metrics(h, topk=(1, 3))
    assert set(got) == set(want) and "top3_2to1" in got and all(torch.equal(got[k], want[k]) for k in want)
