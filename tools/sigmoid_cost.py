#!/usr/bin/env python3
"""What the pairwise sigmoid loss costs: ``ntxent_amd.sigmoid_loss(h)`` + backward against the eager
PyTorch (SigLIP) formulation of the same loss, on one GPU, in one process.

  python tools/sigmoid_cost.py [--out profiles/sigmoid/sigmoid_cost.json] [--iters 30] [--rounds 3]

Shapes: the headline (B = 4096 per view, d = 2048, bf16) and config 2 (B = 4096, d = 512).
Per shape three arms are timed, forward + backward, with device events after warm-up, alternating
in rounds so that drift hits them alike:
  op        ntxent_amd.sigmoid_loss(h) + backward  (row prologue, N x N tile GEMM with the softplus
            epilogue; coefficient block, two MFMA products, normalisation backward; compute "auto")
  eager     F.normalize, A @ B.T / tau + bias, F.logsigmoid, + backward: materialises the N x N logits
            and makes several passes over them
  info_nce  ntxent_amd.info_nce_loss(h) + backward on the same rows, for scale: the same GEMMs with
            the LSE epilogue and merge
``op_forward`` (the op's forward alone, no graph) splits the op's time into forward and backward.
The document records the median, mean, min and max per arm in ms, the ratios, the
torch.cuda.max_memory_allocated deltas of one forward + backward of ``op`` and ``eager``, and how
far the two losses are apart. No speed threshold: the op shares InfoNCE's plain one-tile-per-workgroup
GEMMs and may not beat eager.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = [("headline", 4096, 2048), ("config2", 4096, 512)]
TAU, BIAS = 0.1, -10.0


def eager_siglip(h: torch.Tensor) -> torch.Tensor:
    n = h.shape[0] // 2
    a, b = F.normalize(h[:n], dim=1), F.normalize(h[n:], dim=1)
    logits = a @ b.t() / TAU + BIAS
    s = 2.0 * torch.eye(n, device=h.device, dtype=logits.dtype) - 1.0
    return -F.logsigmoid(s * logits).sum() / n


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


def peak_delta(fn) -> int:
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sigmoid" / "sigmoid_cost.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sigmoid_cost: needs a GPU (no CPU fall-back: a CPU time says nothing here)")
    import ntxent_amd

    dev = torch.device("cuda", 0)
    doc = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "temperature": TAU, "bias": BIAS,
           "iters": args.iters, "rounds": args.rounds, "shapes": {}}
    for name, batch, dim in SHAPES:
        g = torch.Generator().manual_seed(0)
        h1 = torch.randn(batch, dim, generator=g)
        s = 1.5 * torch.rand(batch, 1, generator=g)
        h = torch.cat([h1, s * h1 + torch.randn(batch, dim, generator=g)], 0).to(dev, torch.bfloat16)
        x = h.clone().requires_grad_(True)

        def fwd_bwd(loss_fn):
            def run():
                x.grad = None
                loss_fn(x).backward()
            return run

        def op_forward():
            with torch.no_grad():
                ntxent_amd.sigmoid_loss(h, TAU, BIAS)

        arms = {
            "op": fwd_bwd(lambda t: ntxent_amd.sigmoid_loss(t, TAU, BIAS)),
            "eager": fwd_bwd(eager_siglip),
            "info_nce": fwd_bwd(lambda t: ntxent_amd.info_nce_loss(t, TAU)),
            "op_forward": op_forward,
        }
        for fn in arms.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                ms[k] += time_arm(fn, args.iters)
        x.grad = None
        mem = {k: peak_delta(arms[k]) for k in ("op", "eager")}
        with torch.no_grad():
            l_op, l_eager = float(ntxent_amd.sigmoid_loss(h, TAU, BIAS)), float(eager_siglip(h))
        rec = {k: summary(v) for k, v in ms.items()}
        rec.update(batch=batch, dim=dim, rows=2 * batch,
                   op_over_eager=rec["op"]["median_ms"] / rec["eager"]["median_ms"],
                   op_over_info_nce=rec["op"]["median_ms"] / rec["info_nce"]["median_ms"],
                   op_backward_median_ms=rec["op"]["median_ms"] - rec["op_forward"]["median_ms"],
                   peak_bytes_op=mem["op"], peak_bytes_eager=mem["eager"], loss_op=l_op, loss_eager=l_eager)
        doc["shapes"][name] = rec
        print(f"{name}: op {rec['op']['median_ms']:.4f} ms (forward {rec['op_forward']['median_ms']:.4f}), eager "
              f"{rec['eager']['median_ms']:.4f} ms, info_nce {rec['info_nce']['median_ms']:.4f} ms (medians); op/eager "
              f"{rec['op_over_eager']:.3f}; peak MiB op {mem['op'] / 2**20:.1f}, eager {mem['eager'] / 2**20:.1f}; "
              f"loss op {l_op:.6f} eager {l_eager:.6f}", flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
