#!/usr/bin/env python3
"""Digests of what the cross-view InfoNCE and positive-rank kernels compute, for checking a refactor
bit for bit: run this on two builds on the same machine, one process per build, and compare.

  python tools/xview_digest.py     (loads the build of the checkout it lies in: copy it into the other)

One line per output: SHA-256 (first 16 hex digits) of its raw bytes, for seeded fp32 inputs built
with a CPU torch.Generator, in a fixed order:
  info_nce   loss, dh, dL/dtau of ``info_nce_loss`` (tau = 0.07 as a tensor that requires grad)
  pos_rank   rank, pos_cos, hard_neg_cos of ``positive_rank``
  xview_dist loss and every rank's dh of ``emulated_xview_forward_backward``
  sigmoid    loss, dh, dL/dtau, dL/dbias of ``sigmoid_loss`` (tau = 0.1, bias = -10 as tensors that require grad)
  sigmoid_dist loss, dL/dtau, dL/dbias and every rank's dh of ``emulated_sigmoid_forward_backward``
             (a build without the distributed sigmoid loss prints none of these lines)
  sigmoid_ring the same of ``emulated_sigmoid_forward_backward(..., exchange="ring")``
             (a build without the ring exchange prints none of these lines)
"""
from __future__ import annotations

import hashlib
import inspect
import sys
from pathlib import Path

import torch

ONE_GPU = [(37, 40), (129, 160), (384, 256), (1024, 512)]  # (N pairs, d)
COMPUTES = ["fp32", "fp16", "bf16"]
DIST = [(2, 37, 40, "fp32"), (3, 129, 160, "fp32"), (3, 129, 160, "fp16"), (2, 200, 100, "bf16"), (8, 37, 40, "fp16")]
TAU = 0.07
SIG_TAU, SIG_BIAS = 0.1, -10.0


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def rows(n: int, d: int, seed: int) -> torch.Tensor:
    """Stacked views [2n, d]: the second view is a scaled, noisy copy of the first."""
    g = torch.Generator().manual_seed(seed)
    h1 = torch.randn(n, d, generator=g)
    s = 1.5 * torch.rand(n, 1, generator=g) - 0.25
    return torch.cat([h1, s * h1 + torch.randn(n, d, generator=g)], 0)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("xview_digest: needs a GPU (no CPU fall-back: the digests are the kernels')")
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import ntxent_amd
    from ntxent_amd.ops import _ext
    from ntxent_amd.parallel.emulate import emulated_xview_forward_backward

    print(f"# build {_ext.load(build_if_missing=False).__file__}")
    dev = torch.device("cuda", 0)
    for n, d in ONE_GPU:
        h = rows(n, d, 1000 * n + d).to(dev)
        for comp in COMPUTES:
            x = h.clone().requires_grad_(True)
            tau = torch.tensor(TAU, device=dev, requires_grad=True)
            loss = ntxent_amd.info_nce_loss(x, tau, compute=comp)
            dh, dtau = torch.autograd.grad(loss, (x, tau))
            print(f"info_nce N={n} d={d} {comp}: loss {digest(loss)} dh {digest(dh)} dtau {digest(dtau)}")
            rank, pos, hard = ntxent_amd.positive_rank(h, compute=comp)
            print(f"pos_rank N={n} d={d} {comp}: rank {digest(rank)} pos_cos {digest(pos)} hard_neg_cos {digest(hard)}")
    for W, n, d, comp in DIST:
        shards = [rows(n, d, 1000 * n + d + 101 * r).to(dev) for r in range(W)]
        loss, grads = emulated_xview_forward_backward(shards, TAU, compute=comp, grad_out=0.7)
        print(f"xview_dist W={W} n={n} d={d} {comp}: loss {digest(loss)} " +
              " ".join(f"dh{r} {digest(g)}" for r, g in enumerate(grads)))
    for n, d in ONE_GPU:
        h = rows(n, d, 1000 * n + d).to(dev)
        for comp in COMPUTES:
            x = h.clone().requires_grad_(True)
            tau = torch.tensor(SIG_TAU, device=dev, requires_grad=True)
            bias = torch.tensor(SIG_BIAS, device=dev, requires_grad=True)
            loss = ntxent_amd.sigmoid_loss(x, tau, bias, compute=comp)
            dh, dtau, dbias = torch.autograd.grad(loss, (x, tau, bias))
            print(f"sigmoid N={n} d={d} {comp}: loss {digest(loss)} dh {digest(dh)} dtau {digest(dtau)} dbias {digest(dbias)}")
    try:
        from ntxent_amd.parallel.emulate import emulated_sigmoid_forward_backward
    except ImportError:
        emulated_sigmoid_forward_backward = None
    exchanges = [("sigmoid_dist", {})] if emulated_sigmoid_forward_backward else []
    if exchanges and "exchange" in inspect.signature(emulated_sigmoid_forward_backward).parameters:
        exchanges.append(("sigmoid_ring", {"exchange": "ring"}))
    for name, kw in exchanges:
        for W, n, d, comp in DIST:
            shards = [rows(n, d, 1000 * n + d + 101 * r).to(dev) for r in range(W)]
            loss, grads, dtau, dbias = emulated_sigmoid_forward_backward(shards, SIG_TAU, SIG_BIAS, compute=comp,
                                                                         grad_out=0.7, **kw)
            print(f"{name} W={W} n={n} d={d} {comp}: loss {digest(loss)} dtau {digest(dtau)} dbias {digest(dbias)} " +
                  " ".join(f"dh{r} {digest(g)}" for r, g in enumerate(grads)))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
