#!/usr/bin/env python3
"""What the cross-view InfoNCE op costs: ``ntxent_amd.info_nce_loss(h)`` + backward against the eager
PyTorch (CLIP) formulation of the same loss, on one GPU, in one process.

  python tools/xview_cost.py [--out profiles/infonce/xview_cost.json] [--iters 30] [--rounds 3]

Shapes: the headline (B = 4096 per view, d = 2048, bf16) and config 2 (B = 4096, d = 512).
Per shape three arms are timed, forward + backward, with device events after warm-up, alternating
in rounds so that drift hits them alike:
  op      ntxent_amd.info_nce_loss(h) + backward   (row prologue, N x N tile GEMM with the LSE epilogue,
          merge; coefficient block, two MFMA products, normalisation backward; compute "auto")
  eager   F.normalize, A @ B.T / tau, two F.cross_entropy, + backward: materialises the N x N logits
          and makes several passes over them
  ntxent  ntxent_amd.ntxent_loss(h) + backward on the same rows, for scale: twice the GEMM work
``op_forward`` (the op's forward alone, no graph) splits the op's time into forward and backward.
The document records the median, mean, min and max per arm in ms, the ratios, the
torch.cuda.max_memory_allocated deltas of one forward + backward of ``op`` and ``eager``, and how
far the two losses are apart.

  python tools/xview_cost.py --world W [--out profiles/infonce/xview_cost_wW.json]

times one virtual rank of the distributed form (``ntxent_amd.parallel.dist_info_nce_loss``) instead:
its forward + backward stage ops against gathered buffers filled on the device (no collective is
timed), B = 4096 per view and rank, against the eager PyTorch expression of the same per-rank work,
with the per-rank peak memory of both beside the gathered buffers (``world_cost``).
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
TAU = 0.07


def eager_clip(h: torch.Tensor) -> torch.Tensor:
    n = h.shape[0] // 2
    a, b = F.normalize(h[:n], dim=1), F.normalize(h[n:], dim=1)
    logits = a @ b.t() / TAU
    t = torch.arange(n, device=h.device)
    return 0.5 * F.cross_entropy(logits, t) + 0.5 * F.cross_entropy(logits.t(), t)


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


def world_cost(args, dev):
    """--world W: ONE virtual rank's forward + backward stage ops of the distributed form
    (parallel/infonce.py: prep into its slot, both n x N blocks, merge; transposes, per side the
    coefficient block and its dZ rows, normalisation backward) against gathered buffers that are
    filled on the device, so no collective is timed. B = 4096 per view and rank. The eager arm is the
    same per-rank work in PyTorch: a_r B_all^T, b_r A_all^T, two cross entropies, autograd."""
    from ntxent_amd.ops import _ext
    from ntxent_amd.parallel.infonce import xview_stage_forward

    C = _ext.load()
    W, r = args.world, args.world // 2
    doc = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "temperature": TAU, "iters": args.iters,
           "rounds": args.rounds, "world": W, "rank": r, "shapes": {}}
    for name, batch, dim in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        plans = [C.get_plan(2 * batch, dim, W, q, TAU, "bf16", dev.index) for q in range(W)]
        plan, Rpad = plans[r], plans[r].rows_pad
        zq_all = torch.empty((W * Rpad, plan.ld_k), dtype=torch.bfloat16, device=dev)
        lse2_all = torch.empty((W * Rpad,), dtype=torch.float32, device=dev)
        hs = []
        for q in range(W):  # every slot: a rank's unit rows, then its LSE (device-filled "gathers")
            h1 = torch.randn(batch, dim, generator=g, device=dev)
            s = 1.5 * torch.rand(batch, 1, generator=g, device=dev)
            hs.append(torch.cat([h1, s * h1 + torch.randn(batch, dim, generator=g, device=dev)], 0).bfloat16())
            C.prep(hs[q], plans[q], zq_all[q * Rpad:(q + 1) * Rpad], None)
        for q in range(W):
            ypos = torch.empty((2 * batch,), dtype=torch.float32, device=dev)
            xview_stage_forward(C, plans[q], zq_all, ypos, lse2_all)
        h = hs[r]
        go = torch.ones(1, dtype=torch.float32, device=dev)
        mine = zq_all[r * Rpad:(r + 1) * Rpad]

        def op_forward():
            _, inv, ypos, _ = C.prep(h, plan, mine, None)
            share, cpos = xview_stage_forward(C, plan, zq_all, ypos, lse2_all)
            return inv, cpos, share

        def op():
            inv, cpos, _ = op_forward()
            return C.xview_dist_backward(h, zq_all, inv, lse2_all, cpos, go, plan)

        zf = [F.normalize(x.float(), dim=1).bfloat16() for x in hs]  # the other ranks' unit rows: constants
        x = h.clone().requires_grad_(True)
        target = torch.arange(batch, device=dev) + r * batch

        def eager():
            x.grad = None
            a, b = F.normalize(x[:batch], dim=1), F.normalize(x[batch:], dim=1)
            a_all = torch.cat([a if q == r else zf[q][:batch] for q in range(W)], 0)
            b_all = torch.cat([b if q == r else zf[q][batch:] for q in range(W)], 0)
            loss = (F.cross_entropy(a @ b_all.t() / TAU, target, reduction="sum")
                    + F.cross_entropy(b @ a_all.t() / TAU, target, reduction="sum")) / (2 * W * batch)
            loss.backward()
            return loss

        arms = {"op": op, "eager": eager, "op_forward": op_forward}
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
        rec = {k: summary(v) for k, v in ms.items()}
        rec.update(batch=batch, dim=dim, rows=2 * batch, world=W,
                   op_over_eager=rec["op"]["median_ms"] / rec["eager"]["median_ms"],
                   op_backward_median_ms=rec["op"]["median_ms"] - rec["op_forward"]["median_ms"],
                   peak_bytes_op=mem["op"], peak_bytes_eager=mem["eager"],
                   gathered_bytes=zq_all.numel() * 2 + lse2_all.numel() * 4, coef_bytes=C.xview_dist_coef_bytes(plan),
                   share_op=float(op_forward()[2]), share_eager=float(eager().detach()))
        doc["shapes"][name] = rec
        print(f"W={W} {name}: op {rec['op']['median_ms']:.4f} ms (forward {rec['op_forward']['median_ms']:.4f}), eager "
              f"{rec['eager']['median_ms']:.4f} ms (medians); op/eager {rec['op_over_eager']:.3f}; peak MiB op "
              f"{mem['op'] / 2**20:.1f}, eager {mem['eager'] / 2**20:.1f} (beside {rec['gathered_bytes'] / 2**20:.1f} "
              f"gathered); loss share op {rec['share_op']:.6f} eager {rec['share_eager']:.6f}", flush=True)
        del zq_all, zf, hs
        torch.cuda.empty_cache()
    return doc


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/infonce/xview_cost.json (xview_cost_wW.json with --world)")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--world", type=int, default=1,
                    help="W > 1: one virtual rank of the distributed form against device-filled gathered buffers")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("xview_cost: needs a GPU (no CPU fall-back: a CPU time says nothing here)")
    import ntxent_amd

    dev = torch.device("cuda", 0)
    if args.out is None:
        args.out = str(ROOT / "profiles" / "infonce" / (f"xview_cost_w{args.world}.json" if args.world > 1 else "xview_cost.json"))
    if args.world > 1:
        doc = world_cost(args, dev)
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(doc, indent=1) + "\n")
        print(f"wrote {out}")
        return
    doc = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "temperature": TAU, "iters": args.iters,
           "rounds": args.rounds, "shapes": {}}
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
                ntxent_amd.info_nce_loss(h, TAU)

        arms = {
            "op": fwd_bwd(lambda t: ntxent_amd.info_nce_loss(t, TAU)),
            "eager": fwd_bwd(eager_clip),
            "ntxent": fwd_bwd(lambda t: ntxent_amd.ntxent_loss(t, TAU)),
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
            l_op, l_eager = float(ntxent_amd.info_nce_loss(h, TAU)), float(eager_clip(h))
        rec = {k: summary(v) for k, v in ms.items()}
        rec.update(batch=batch, dim=dim, rows=2 * batch,
                   op_over_eager=rec["op"]["median_ms"] / rec["eager"]["median_ms"],
                   op_over_ntxent=rec["op"]["median_ms"] / rec["ntxent"]["median_ms"],
                   op_backward_median_ms=rec["op"]["median_ms"] - rec["op_forward"]["median_ms"],
                   peak_bytes_op=mem["op"], peak_bytes_eager=mem["eager"], loss_op=l_op, loss_eager=l_eager)
        doc["shapes"][name] = rec
        print(f"{name}: op {rec['op']['median_ms']:.4f} ms (forward {rec['op_forward']['median_ms']:.4f}), eager "
              f"{rec['eager']['median_ms']:.4f} ms, ntxent {rec['ntxent']['median_ms']:.4f} ms (medians); op/eager "
              f"{rec['op_over_eager']:.3f}; peak MiB op {mem['op'] / 2**20:.1f}, eager {mem['eager'] / 2**20:.1f}",
              flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
