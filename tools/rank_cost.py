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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "metrics" / "rank_cost.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rank_cost: needs a GPU (no CPU fall-back: a CPU time says nothing here)")
    import ntxent_amd

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


if __name__ == "__main__":
    main()
