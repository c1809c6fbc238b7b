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

  python tools/sigmoid_cost.py --world W [--out profiles/sigmoid_dist/sigmoid_cost_wW.json]

times one virtual rank of the distributed form (``ntxent_amd.parallel.dist_sigmoid_loss``) instead: its
forward + backward stage ops, both scalar gradients wanted, against gathered rows filled on the
device (no collective is timed), B = 4096 per view and rank, d = 512 and 2048, fp16. Three arms in the
same run: the op; the eager PyTorch expression of the same per-rank work in the same arithmetic
(fp16 unit rows and matmuls, fp32 elementwise: a_r B_all^T forward, both sides through autograd);
and one rank of ``dist_info_nce_loss`` on the same rows. ``--memory`` records instead the
torch.cuda.max_memory_allocated delta of one emulated rank's step at W = 2, n = 1024, d = 512, fp16,
for both losses.

  python tools/sigmoid_cost.py --world W --exchange ring [--out profiles/sigmoid_ring/sigmoid_cost_wW.json]

times one virtual rank's stage ops of ``exchange="ring"`` beside the gather ones, in one process, in
alternating rounds, on the same device-filled rows, and records both modes' peak bytes.
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


WORLD_SHAPES = [("d512", 4096, 512), ("d2048", 4096, 2048)]


def _rank_setup(C, W, batch, dim, dev, dtype=torch.float16, comp="fp16", tau=TAU):
    """Plans, this process's virtual ranks' rows and zq_all with every slot filled by its rank's prep."""
    g = torch.Generator(device=dev).manual_seed(0)
    plans = [C.get_plan(2 * batch, dim, W, q, tau, comp, dev.index) for q in range(W)]
    Rpad = plans[0].rows_pad
    zq_all = torch.empty((W * Rpad, plans[0].ld_k), dtype=dtype, device=dev)
    hs = []
    for q in range(W):
        h1 = torch.randn(batch, dim, generator=g, device=dev)
        s = 1.5 * torch.rand(batch, 1, generator=g, device=dev)
        hs.append(torch.cat([h1, s * h1 + torch.randn(batch, dim, generator=g, device=dev)], 0).to(dtype))
        C.prep(hs[q], plans[q], zq_all[q * Rpad:(q + 1) * Rpad], None)
    return plans, hs, zq_all, Rpad


def _rank_steps(C, plans, hs, zq_all, Rpad, r, dev):
    """(sigmoid rank step, InfoNCE rank step, sigmoid forward alone) of virtual rank r as closures."""
    from ntxent_amd.parallel.infonce import xview_stage_forward
    from ntxent_amd.parallel.sigmoid import sigmoid_stage_forward

    W = len(plans)
    plan, h = plans[r], hs[r]
    mine = zq_all[r * Rpad:(r + 1) * Rpad]
    go = torch.ones(1, dtype=torch.float32, device=dev)
    lse2_all = torch.empty((W * Rpad,), dtype=torch.float32, device=dev)
    for q in range(W):  # the other ranks' LSE: a device-filled "gather"
        xview_stage_forward(C, plans[q], zq_all, torch.empty((h.shape[0],), dtype=torch.float32, device=dev), lse2_all)

    def op_forward():
        _, inv, _, _ = C.prep(h, plan, mine, None)
        return inv, sigmoid_stage_forward(C, plan, zq_all, h, inv, BIAS)

    def op():
        inv, _ = op_forward()
        return C.xview_sigmoid_dist_backward(h, zq_all, inv, go, plan, BIAS, True, True)

    def info_nce():
        _, inv, ypos, _ = C.prep(h, plan, mine, None)
        _, cpos = xview_stage_forward(C, plan, zq_all, ypos, lse2_all)
        return C.xview_dist_backward(h, zq_all, inv, lse2_all, cpos, go, plan)

    return op, info_nce, op_forward


def world_cost(args, dev):
    from ntxent_amd.ops import _ext

    C = _ext.load()
    W, r = args.world, args.world // 2
    doc = {"device": torch.cuda.get_device_name(0), "dtype": "fp16", "temperature": TAU, "bias": BIAS,
           "iters": args.iters, "rounds": args.rounds, "world": W, "rank": r, "shapes": {}}
    for name, batch, dim in WORLD_SHAPES:
        plans, hs, zq_all, Rpad = _rank_setup(C, W, batch, dim, dev)
        op, info_nce, op_forward = _rank_steps(C, plans, hs, zq_all, Rpad, r, dev)
        zf = [F.normalize(x.float(), dim=1).half() for x in hs]  # the other ranks' unit rows: constants
        x = hs[r].clone().requires_grad_(True)
        N = W * batch
        sign = -torch.ones(batch, N, device=dev)
        sign[torch.arange(batch), torch.arange(batch) + r * batch] = 1.0

        a_oth = torch.cat([zf[q][:batch] for q in range(W) if q != r], 0)

        def eager():
            # the rank's forward block a_r B_all^T (b_r live in its own slot), and for the rest of b_r's
            # gradient its pairs with the a of the other ranks (all negatives): every pair once
            x.grad = None
            z = F.normalize(x.float(), dim=1).half()
            a, b = z[:batch], z[batch:]
            b_all = torch.cat([b if q == r else zf[q][batch:] for q in range(W)], 0)
            fwd = F.softplus(-sign * ((a @ b_all.t()).float() / TAU + BIAS)).sum() / N
            other = F.softplus((b @ a_oth.t()).float() / TAU + BIAS).sum() / N
            (fwd + other).backward()
            return fwd

        arms = {"op": op, "eager": eager, "info_nce": info_nce, "op_forward": op_forward}
        for fn in arms.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                ms[k] += time_arm(fn, args.iters)
        x.grad = None
        mem = {k: peak_delta(arms[k]) for k in ("op", "eager", "info_nce")}
        rec = {k: summary(v) for k, v in ms.items()}
        rec.update(batch=batch, dim=dim, rows=2 * batch, world=W,
                   op_over_eager=rec["op"]["median_ms"] / rec["eager"]["median_ms"],
                   op_over_info_nce=rec["op"]["median_ms"] / rec["info_nce"]["median_ms"],
                   op_backward_median_ms=rec["op"]["median_ms"] - rec["op_forward"]["median_ms"],
                   peak_bytes_op=mem["op"], peak_bytes_eager=mem["eager"], peak_bytes_info_nce=mem["info_nce"],
                   gathered_bytes=zq_all.numel() * 2, share_op=float(op_forward()[1]), share_eager=float(eager().detach()))
        doc["shapes"][name] = rec
        print(f"W={W} {name}: op {rec['op']['median_ms']:.4f} ms (forward {rec['op_forward']['median_ms']:.4f}), eager "
              f"{rec['eager']['median_ms']:.4f} ms, info_nce rank {rec['info_nce']['median_ms']:.4f} ms (medians); op/eager "
              f"{rec['op_over_eager']:.3f}, op/info_nce {rec['op_over_info_nce']:.3f}; peak MiB op {mem['op'] / 2**20:.1f}, "
              f"eager {mem['eager'] / 2**20:.1f}, info_nce {mem['info_nce'] / 2**20:.1f} (beside "
              f"{rec['gathered_bytes'] / 2**20:.1f} gathered); loss share op {rec['share_op']:.6f} eager "
              f"{rec['share_eager']:.6f}", flush=True)
        del zq_all, zf, hs, plans, op, info_nce, op_forward, a_oth, sign
        torch.cuda.empty_cache()
    return doc


def ring_cost(args, dev):
    """``--world W --exchange ring``: one virtual rank's forward + backward stage ops of both exchanges in
    one process, in alternating rounds, on the same device-filled rows (no transfer is timed: the ring's
    blocks are the other ranks' slots, visited in ring order). Medians, and the peak bytes of one step
    of each above the rows that are there before it (the gather's W slots, of which the ring needs its
    own and two buffers)."""
    from ntxent_amd.ops import _ext
    from ntxent_amd.parallel.sigmoid import (sigmoid_ring_stage_backward, sigmoid_ring_stage_forward,
                                             sigmoid_stage_forward)

    C = _ext.load()
    W, r = args.world, args.world // 2
    doc = {"device": torch.cuda.get_device_name(0), "dtype": "fp16", "temperature": TAU, "bias": BIAS,
           "iters": args.iters, "rounds": args.rounds, "world": W, "rank": r, "shapes": {}}
    for name, batch, dim in WORLD_SHAPES:
        plans, hs, zq_all, Rpad = _rank_setup(C, W, batch, dim, dev)
        plan, h = plans[r], hs[r]
        slots = [zq_all[q * Rpad:(q + 1) * Rpad] for q in range(W)]
        go = torch.ones(1, dtype=torch.float32, device=dev)

        def visit(fn):
            for s in range(W):
                fn((r - s) % W, slots[(r - s) % W], 0)

        def gather_forward():
            _, inv, _, _ = C.prep(h, plan, slots[r], None)
            return inv, sigmoid_stage_forward(C, plan, zq_all, h, inv, BIAS)

        def gather():
            inv, _ = gather_forward()
            return C.xview_sigmoid_dist_backward(h, zq_all, inv, go, plan, BIAS, True, True)

        def ring_forward():
            _, inv, _, _ = C.prep(h, plan, slots[r], None)
            return inv, sigmoid_ring_stage_forward(C, plan, slots[r], h, inv, BIAS, visit)

        def ring():
            inv, _ = ring_forward()
            return sigmoid_ring_stage_backward(C, plan, slots[r], h, inv, BIAS, go, True, True, visit)

        arms = {"gather": gather, "ring": ring, "gather_forward": gather_forward, "ring_forward": ring_forward}
        for fn in arms.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                ms[k] += time_arm(fn, args.iters)
        mem = {k: peak_delta(arms[k]) for k in ("gather", "ring")}
        slot_bytes = Rpad * plan.ld_k * 2
        rec = {k: summary(v) for k, v in ms.items()}
        dg, dr = gather(), ring()
        rec.update(batch=batch, dim=dim, rows=2 * batch, world=W,
                   ring_over_gather=rec["ring"]["median_ms"] / rec["gather"]["median_ms"],
                   ring_forward_over_gather_forward=rec["ring_forward"]["median_ms"] / rec["gather_forward"]["median_ms"],
                   stage_peak_bytes_gather=mem["gather"], stage_peak_bytes_ring=mem["ring"], slot_bytes=slot_bytes,
                   # with the rows each mode holds: W slots, or the own slot and two ring buffers
                   rank_peak_bytes_gather=mem["gather"] + W * slot_bytes, rank_peak_bytes_ring=mem["ring"] + 3 * slot_bytes,
                   bytes_across_ranks_gather=(W - 1) * slot_bytes, bytes_across_ranks_ring=2 * (W - 1) * slot_bytes,
                   loss_share_equal=bool(torch.equal(gather_forward()[1], ring_forward()[1])),
                   dbias_share_equal=bool(torch.equal(dg[1][1], dr[1][1])),
                   dh_max_abs_diff=float((dg[0].float() - dr[0].float()).abs().max()))
        doc["shapes"][name] = rec
        print(f"W={W} {name}: gather {rec['gather']['median_ms']:.4f} ms (forward {rec['gather_forward']['median_ms']:.4f}), "
              f"ring {rec['ring']['median_ms']:.4f} ms (forward {rec['ring_forward']['median_ms']:.4f}) (medians); "
              f"ring/gather {rec['ring_over_gather']:.3f}; stage peak MiB gather {mem['gather'] / 2**20:.1f} ring "
              f"{mem['ring'] / 2**20:.1f}; with rows gather {rec['rank_peak_bytes_gather'] / 2**20:.1f} ring "
              f"{rec['rank_peak_bytes_ring'] / 2**20:.1f}; loss share equal {rec['loss_share_equal']}, dbias share equal "
              f"{rec['dbias_share_equal']}", flush=True)
        del zq_all, hs, plans, slots, dg, dr, arms
        torch.cuda.empty_cache()
    return doc


def memory_record(dev):
    """torch.cuda.max_memory_allocated delta of one emulated rank's step (prep into its slot, forward,
    backward) at W = 2, n = 1024, d = 512, fp16, beside zq_all: the sigmoid loss and InfoNCE."""
    from ntxent_amd.ops import _ext

    C = _ext.load()
    plans, hs, zq_all, Rpad = _rank_setup(C, 2, 1024, 512, dev)
    op, info_nce, _ = _rank_steps(C, plans, hs, zq_all, Rpad, 1, dev)
    for fn in (op, info_nce):
        fn()
    doc = {"world": 2, "n": 1024, "dim": 512, "dtype": "fp16", "peak_bytes_sigmoid": peak_delta(op),
           "peak_bytes_info_nce": peak_delta(info_nce), "gathered_bytes": zq_all.numel() * 2}
    print(f"one emulated rank's step, W=2 n=1024 d=512 fp16: peak bytes sigmoid {doc['peak_bytes_sigmoid']}, "
          f"info_nce {doc['peak_bytes_info_nce']} (beside {doc['gathered_bytes']} gathered)")
    return doc


def _write(doc, out):
    out = Path(out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {out}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/sigmoid/sigmoid_cost.json (profiles/sigmoid_dist/"
                    "sigmoid_cost_wW.json with --world, memory.json with --memory)")
    ap.add_argument("--world", type=int, default=1,
                    help="W > 1: one virtual rank of the distributed form against device-filled gathered rows")
    ap.add_argument("--exchange", choices=["gather", "ring"], default="gather",
                    help="with --world: ring times the ring stage ops beside the gather ones in alternating rounds")
    ap.add_argument("--memory", action="store_true", help="record one emulated rank's peak memory (W = 2) instead")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sigmoid_cost: needs a GPU (no CPU fall-back: a CPU time says nothing here)")
    import ntxent_amd

    dev = torch.device("cuda", 0)
    if args.exchange == "ring":
        if args.memory or args.world < 2:
            raise SystemExit("sigmoid_cost: --exchange ring goes with --world W, W > 1")
        _write(ring_cost(args, dev), args.out or ROOT / "profiles" / "sigmoid_ring" / f"sigmoid_cost_w{args.world}.json")
        return
    if args.memory or args.world > 1:
        name = "memory.json" if args.memory else f"sigmoid_cost_w{args.world}.json"
        _write(memory_record(dev) if args.memory else world_cost(args, dev),
               args.out or ROOT / "profiles" / "sigmoid_dist" / name)
        return
    args.out = args.out or str(ROOT / "profiles" / "sigmoid" / "sigmoid_cost.json")
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
