"""Contrastive metrics without a GPU: the PyTorch oracles (ops/reference.py), the public functions
on CPU tensors (ops/metrics.py), the module method and the trainer's ``metrics_every``."""
import pytest
import torch

import ntxent_amd
from ntxent_amd.ops import reference as R


def _views(n, d, seed=0, dtype=torch.float64):
    """h1 random, h2 = s * h1 + noise with one s ~ U[0, 1.5] per row: ranks spread from 0 up."""
    g = torch.Generator().manual_seed(seed)
    h1 = torch.randn(n, d, generator=g, dtype=torch.float64)
    s = 1.5 * torch.rand(n, 1, generator=g, dtype=torch.float64)
    h2 = s * h1 + torch.randn(n, d, generator=g, dtype=torch.float64)
    return torch.cat([h1, h2], 0).to(dtype)


def test_oracle_identical_views_rank_zero():
    h1 = _views(19, 12)[:19]
    rank, pos, hard = R.positive_rank(torch.cat([h1, h1], 0))
    assert rank.dtype == torch.int32 and rank.shape == (38,)
    assert (rank == 0).all()
    assert torch.allclose(pos, torch.ones_like(pos))
    assert (hard < 1).all()


def test_oracle_opposite_views_rank_last():
    h1 = _views(19, 12)[:19]
    rank, pos, _ = R.positive_rank(torch.cat([h1, -h1], 0))
    assert (rank == 2 * 19 - 2).all()
    assert torch.allclose(pos, -torch.ones_like(pos))


def test_oracle_single_pair_has_no_negatives():
    rank, _, hard = R.positive_rank(_views(1, 8))
    assert (rank == 0).all() and rank.numel() == 2
    assert torch.isinf(hard).all() and (hard < 0).all()


def test_oracle_matches_a_sort():
    """rank = position of the positive among the row's candidates, by an independent formulation."""
    h = _views(23, 10, seed=3)
    rank, pos, hard = R.positive_rank(h)
    z, _ = R.normalize(h)  # the oracle's own unit rows: the comparisons below are then exact
    cos = z @ z.t()
    n = 23
    for i in range(2 * n):
        p = (i + n) % (2 * n)
        others = [j for j in range(2 * n) if j not in (i, p)]
        assert int(rank[i]) == sum(1 for j in others if cos[i, j] > cos[i, p])
        assert float(hard[i]) == max(float(cos[i, j]) for j in others)
        assert float(pos[i]) == float(cos[i, p])
    assert rank.min() == 0 and rank.max() > n // 2  # the data spreads the ranks


def test_oracle_works_in_the_dtype_of_h():
    for dt in (torch.float32, torch.float64):
        _, pos, hard = R.positive_rank(_views(9, 6, dtype=dt))
        assert pos.dtype == dt and hard.dtype == dt


def test_bounds_bracket_the_rank():
    h = _views(40, 16, seed=1)
    z, _ = R.normalize(h)
    rank, _, _ = R.positive_rank(h)
    lo0, hi0 = R.positive_rank_bounds(z, 0.0)
    assert torch.equal(lo0, hi0) and torch.equal(lo0.to(torch.int32), rank)
    lo, hi = R.positive_rank_bounds(z, 0.05)
    assert (lo <= rank).all() and (rank <= hi).all()
    assert (lo < hi).any()  # a bracket this wide is not tight on 80 rows


def test_contrastive_metrics_on_cpu():
    n = 33
    h = _views(n, 20, seed=2, dtype=torch.float32)
    rank, pos, hard = ntxent_amd.positive_rank(h)
    ref = R.positive_rank(h)
    assert torch.equal(rank, ref[0]) and rank.dtype == torch.int32
    assert pos.dtype == torch.float32 and hard.dtype == torch.float32
    m = ntxent_amd.contrastive_metrics(h)
    assert set(m) == {"top1", "top5", "mean_rank", "pos_cos", "hard_neg_cos", "negatives"}
    assert all(v.dim() == 0 and v.device == h.device for v in m.values())
    assert float(m["top1"]) == float((rank == 0).float().mean())
    assert float(m["top5"]) == float((rank < 5).float().mean())
    assert float(m["top5"]) >= float(m["top1"])
    assert float(m["mean_rank"]) == float(rank.float().mean())
    assert int(m["negatives"]) == 2 * n - 2
    assert float(m["pos_cos"]) == float(pos.mean()) and float(m["hard_neg_cos"]) == float(hard.mean())
    m3 = ntxent_amd.contrastive_metrics(h[:n], z2=h[n:], topk=(3,))
    assert set(m3) == {"top3", "mean_rank", "pos_cos", "hard_neg_cos", "negatives"}
    assert float(m3["top3"]) == float((rank < 3).float().mean())


def test_metrics_run_without_grad():
    h = _views(8, 6, dtype=torch.float32).requires_grad_(True)
    m = ntxent_amd.contrastive_metrics(h)
    assert not any(v.requires_grad for v in m.values())
    assert not any(t.requires_grad for t in ntxent_amd.positive_rank(h))


def test_input_validation():
    with pytest.raises(ValueError):
        ntxent_amd.positive_rank(torch.randn(7, 4))
    with pytest.raises(ValueError):
        ntxent_amd.contrastive_metrics(torch.randn(7, 4))
    with pytest.raises(ValueError):
        ntxent_amd.positive_rank(torch.randn(8))
    with pytest.raises(ValueError):
        ntxent_amd.positive_rank(torch.randn(8, 4), compute="int4")
    with pytest.raises(ValueError):
        ntxent_amd.contrastive_metrics(torch.randn(8, 4), topk=(0,))
    with pytest.raises(ValueError):
        R.positive_rank(torch.randn(7, 4))


def test_module_metrics_match_the_function():
    h = _views(12, 8, seed=4, dtype=torch.float32)
    got = ntxent_amd.NTXentLoss(0.2).metrics(h[:12], h[12:])
    want = ntxent_amd.contrastive_metrics(h)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    got3 = ntxent_amd.NTXentLoss(0.2).metrics(h, topk=(3,))
    assert "top3" in got3 and "top1" not in got3


def test_package_surface():
    from ntxent_amd import ops
    from ntxent_amd.ops import metrics

    for name in ("positive_rank", "contrastive_metrics"):
        assert getattr(ntxent_amd, name) is getattr(metrics, name)
        assert getattr(ops, name) is getattr(metrics, name)
    assert callable(R.positive_rank) and callable(R.positive_rank_bounds)


def _trainer(tmp_path, **kw):
    from ntxent_amd.models.trainer import SimCLRTrainer, TrainConfig

    cfg = TrainConfig(steps=3, batch=16, image_size=8, encoder="mlp", proj_hidden=32, proj_out=16, temperature=0.5,
                      optimizer="lars", lr=0.5, warmup_steps=1, amp=False, log_every=0, ckpt_dir=str(tmp_path),
                      ckpt_every=3, **kw)
    return SimCLRTrainer(cfg, device=torch.device("cpu"))


METRIC_KEYS = {"top1", "top5", "mean_rank", "pos_cos", "hard_neg_cos", "negatives"}


def test_trainer_metrics_every(tmp_path):
    from ntxent_amd.utils.checkpoint import latest_checkpoint

    hist = _trainer(tmp_path, metrics_every=2).fit()
    assert len(hist) == 3
    base = {"step", "loss", "lr", "step_ms", "images_per_s"}
    assert set(hist[0]) == base | METRIC_KEYS and set(hist[2]) == base | METRIC_KEYS
    assert set(hist[1]) == base
    for rec in (hist[0], hist[2]):
        assert rec["negatives"] == 2 * 16 - 2 and isinstance(rec["negatives"], int)
        assert all(isinstance(rec[k], float) for k in METRIC_KEYS - {"negatives"})
        assert 0.0 <= rec["top1"] <= rec["top5"] <= 1.0
        assert 0.0 <= rec["mean_rank"] <= rec["negatives"]
        assert -1.0 <= rec["pos_cos"] <= 1.0 + 1e-6 and -1.0 <= rec["hard_neg_cos"] <= 1.0 + 1e-6
    state = torch.load(latest_checkpoint(tmp_path), weights_only=True)
    assert state["extra"]["config"]["metrics_every"] == 2


def test_trainer_metrics_do_not_change_training(tmp_path):
    """The metrics read the step's embeddings and nothing else: same losses with and without."""
    off = _trainer(tmp_path / "off").fit()
    on = _trainer(tmp_path / "on", metrics_every=1).fit()
    assert [r["loss"] for r in off] == [r["loss"] for r in on]
    state = torch.load(sorted((tmp_path / "off").glob("*.pt"))[-1], weights_only=True)
    assert "metrics_every" not in state["extra"]["config"]


def test_metrics_every_defaults_off():
    import dataclasses

    from ntxent_amd.models.trainer import TrainConfig

    f = {x.name: x for x in dataclasses.fields(TrainConfig)}
    assert f["metrics_every"].default == 0
