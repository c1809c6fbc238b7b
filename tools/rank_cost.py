#!/usr/bin/env python3
"""What the contrastive-metrics launch costs: ``ntxent_amd.positive_rank(h)`` against the eager
PyTorch formulation of the same rank, on one GPU, in one process.

  python tools/rank_cost.py [--out profiles/metrics/rank_cost.json] [--iters 30] [--rounds 3]

Shapes: the headline (B = 4096 per view, d = 2048, bf16) and config 2 (B = 4096, d = 512).
Per shape three arms are timed with device events after warm-up, alternating in rounds so that
drift hits them alike:
  op      ntxent_amd.positive_rank(h)            (row prologue + rank kernel; compute "auto")
  eager   normalise, z @ z.T, mask self and the positive, compare against the gathered positive
          cosine, sum(1): materialises the 2N x 2N matrix and makes several passes over it
  loss_forward   ntxent_amd.ntxent_loss(h) forward alone (row prologue, similarity GEMM with the
          LSE epilogue, merge), for scale only
The document records the median, mean, min and max per arm in ms, the ratios, and how many rows the
two formulations rank alike (they round differently: the eager GEMM's cosines are bf16).

  python tools/rank_cost.py --cross-view [--out profiles/retrieval_rank/rank_cost.json]

times ``ntxent_amd.retrieval_rank(h)`` (each view ranked among the other view only, with the hardest
negative's index) at the same shapes instead. Arms:
  op      ntxent_amd.retrieval_rank(h)           (row prologue + cross-view rank kernels)
  eager   normalise, z1 @ z2.T, two comparisons and sums, two masked argmaxes: materialises the N x N
          block and makes several passes over it
  positive_rank   ntxent_amd.positive_rank(h) on the same rows: the upper triangle of 2N x 2N, about
          twice the MFMA work
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = [("headline", 4096, 2048), ("config2", 4096, 512)]


def eager_rank(h: torch.Tensor) -> torch.Tensor:
    rows = h.shape[0]
    z = torch.nn.functional.normalize(h, dim=1)
    cos = z @ z.t()
    idx = torch.arange(rows, device=h.device)
    pos = (idx + rows // 2) % rows
    t = cos.gather(1, pos.unsqueeze(1))
    cos[idx, idx] = float("-inf")
    cos[idx, pos] = float("-inf")
    return (cos > t).sum(1)


def eager_retrieval(h: torch.Tensor):
    """(rank, hard_neg_cos, hard_neg_index), stacked order, by the eager expression of the same outputs."""
    n = h.shape[0] // 2
    z = torch.nn.functional.normalize(h, dim=1)
    S = z[:n] @ z[n:].t()
    t = S.diagonal().clone()
    rank = torch.cat([(S > t.unsqueeze(1)).sum(1), (S > t.unsqueeze(0)).sum(0)])  # the diagonal is never > itself
    S.diagonal().fill_(float("-inf"))
    row, col = S.max(1), S.max(0)
    return rank, torch.cat([row.values, col.values]), torch.cat([row.indices, col.indices])


def time_arm(fn, iters: int):
    a = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
    b = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
    for i in range(iters):
        a[i].record()
        fn()
        b[i].record()
    torch.cuda.synchronize()
    return [x.elapsed_time(y) for x, y in zip(a, b)]


def summary(ms):
    return {"median_ms": statistics.median(ms), "mean_ms": statistics.fmean(ms), "min_ms": min(ms), "max_ms": max(ms),
            "samples": len(ms)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cross-view", action="store_true", help="time retrieval_rank instead of positive_rank")
    ap.add_argument("--out", default=None, help="default: profiles/metrics/rank_cost.json, with --cross-view "
                    "profiles/retrieval_rank/rank_cost.json")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rank_cost: needs a GPU (no CPU fall-back: a CPU time says nothing here)")
    import ntxent_amd

    if args.out is None:
        args.out = str(ROOT / "profiles" / ("retrieval_rank" if args.cross_view else "metrics") / "rank_cost.json")
    if args.cross_view:
        return cross_view(args, ntxent_amd)
    dev = torch.device("cuda", 0)
    doc = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "iters": args.iters, "rounds": args.rounds,
           "shapes": {}}
    for name, batch, dim in SHAPES:
        g = torch.Generator().manual_seed(0)
        h1 = torch.randn(batch, dim, generator=g)
        s = 1.5 * torch.rand(batch, 1, generator=g)
        h = torch.cat([h1, s * h1 + torch.randn(batch, dim, generator=g)], 0).to(dev, torch.bfloat16)
        arms = {
            "op": lambda: ntxent_amd.positive_rank(h),
            "eager": lambda: eager_rank(h),
            "loss_forward": lambda: ntxent_amd.ntxent_loss(h, 0.07),
        }
        with torch.no_grad():
            for fn in arms.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in arms}
            for _ in range(args.rounds):
                for k, fn in arms.items():
                    ms[k] += time_arm(fn, args.iters)
            rank = ntxent_amd.positive_rank(h)[0].long()
            er = eager_rank(h)
        rec = {k: summary(v) for k, v in ms.items()}
        rec.update(batch=batch, dim=dim, rows=2 * batch,
                   op_over_eager=rec["op"]["median_ms"] / rec["eager"]["median_ms"],
                   op_over_loss_forward=rec["op"]["median_ms"] / rec["loss_forward"]["median_ms"],
                   rows_ranked_alike=float((rank == er).float().mean()),
                   top1_op=float((rank == 0).float().mean()), top1_eager=float((er == 0).float().mean()))
        doc["shapes"][name] = rec
        print(f"{name}: op {rec['op']['median_ms']:.4f} ms, eager {rec['eager']['median_ms']:.4f} ms, loss forward "
              f"{rec['loss_forward']['median_ms']:.4f} ms (medians); op/eager {rec['op_over_eager']:.3f}", flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {out}")


def cross_view(args, ntxent_amd):
    dev = torch.device("cuda", 0)
    doc = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "iters": args.iters, "rounds": args.rounds,
           "mode": "cross_view", "shapes": {}}
    for name, batch, dim in SHAPES:
        g = torch.Generator().manual_seed(0)
        h1 = torch.randn(batch, dim, generator=g)
        s = 1.5 * torch.rand(batch, 1, generator=g)
        h = torch.cat([h1, s * h1 + torch.randn(batch, dim, generator=g)], 0).to(dev, torch.bfloat16)
        arms = {
            "op": lambda: ntxent_amd.retrieval_rank(h),
            "eager": lambda: eager_retrieval(h),
            "positive_rank": lambda: ntxent_amd.positive_rank(h),
        }
        with torch.no_grad():
            for fn in arms.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in arms}
            for _ in range(args.rounds):
                for k, fn in arms.items():
                    ms[k] += time_arm(fn, args.iters)
            rank, _, _, index = ntxent_amd.retrieval_rank(h)
            er, _, ei = eager_retrieval(h)
        rec = {k: summary(v) for k, v in ms.items()}
        rec.update(batch=batch, dim=dim, rows=2 * batch,
                   op_over_eager=rec["op"]["median_ms"] / rec["eager"]["median_ms"],
                   op_over_positive_rank=rec["op"]["median_ms"] / rec["positive_rank"]["median_ms"],
                   rows_ranked_alike=float((rank.long() == er).float().mean()),
                   hard_negatives_alike=float((index.long() == ei).float().mean()),
                   top1_op=float((rank == 0).float().mean()), top1_eager=float((er == 0).float().mean()))
        doc["shapes"][name] = rec
        print(f"{name}: op {rec['op']['median_ms']:.4f} ms, eager {rec['eager']['median_ms']:.4f} ms, positive_rank "
              f"{rec['positive_rank']['median_ms']:.4f} ms (medians); op/eager {rec['op_over_eager']:.3f}, "
              f"op/positive_rank {rec['op_over_positive_rank']:.3f}", flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
