"""Single-GPU emulation of the W-rank data-parallel NT-Xent (testing / debugging aid).

Runs every virtual rank's stage ops (the same HIP kernels and per-rank plans the RCCL path
uses: own-rank upper-triangular tiles, remote column blocks with global column indices,
per-rank LSE slot, rank-local symmetric backward) sequentially on one device. The
collectives are replaced by construction: each rank's ``prep``/``transpose`` writes into its
slot of the shared gathered buffers, and each rank's LSE lands in its slot of ``lse2_all``.
This is what lets a 1-GPU box verify the multi-GPU math bit-for-bit (the real path differs
only in who fills the other slots).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from ..ops import _ext
from ..ops.ntxent import resolve_compute


def emulated_dist_forward_backward(shards: Sequence[torch.Tensor], temperature: float, *, compute: str = "auto",
                                   keep_logits: bool = True, grad_out: float = 1.0
                                   ) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """Loss (global mean over all W*R rows) and per-rank dL/dh_r for shards h_r = [h1_r; h2_r]."""
    C = _ext.load()
    W = len(shards)
    R, d = shards[0].shape
    dev = shards[0].device
    comp = resolve_compute(shards[0].dtype, False, compute)
    plans = [C.get_plan(R, d, W, r, float(temperature), comp, dev.index) for r in range(W)]
    P0 = plans[0]
    Rpad = P0.rows_pad
    f8 = P0.compute_dtype == "fp8"
    keep_logits = keep_logits or f8  # fp8 plans always keep their (fp16) cosines
    cdt = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[P0.backward_dtype]
    zq_all = torch.empty((W * Rpad, P0.ld_k), dtype=cdt, device=dev)
    zqt_all = torch.empty((W, P0.dim_n, P0.ld_t), dtype=cdt, device=dev)
    zq8_all = torch.empty((W * Rpad, P0.ld_k8), dtype=torch.uint8, device=dev) if f8 else None
    invs, yposs = [], []
    for r in range(W):  # "all-gather" of Zq / ZqT: every rank writes its own slot
        zq = zq_all[r * Rpad:(r + 1) * Rpad]
        zq8 = zq8_all[r * Rpad:(r + 1) * Rpad] if f8 else None
        _, inv, ypos, _ = C.prep(shards[r].contiguous(), plans[r], zq, zq8)
        C.transpose(zq, plans[r], zqt_all[r])
        invs.append(inv)
        yposs.append(ypos)
    fwd_all = zq8_all if f8 else zq_all  # forward GEMM operand
    lse2_all = torch.empty((W * Rpad,), dtype=torch.float32, device=dev)
    loss = torch.zeros((), dtype=torch.float32, device=dev)
    scs, cposs = [], []
    for r in range(W):
        P = plans[r]
        part = torch.empty((P.col_tiles, Rpad, 2), dtype=torch.float32, device=dev)
        sc = torch.empty((P.n_fwd_tiles * 256 * 256,), dtype=cdt, device=dev) if keep_logits else None
        C.fwd_stats_range(fwd_all[r * Rpad:(r + 1) * Rpad], fwd_all, P, part, sc, 0, P.n_fwd_tiles)
        cpos = torch.empty((Rpad,), dtype=torch.float32, device=dev)
        loss = loss + C.lse(part, yposs[r], lse2_all, cpos, P)  # "all-gather" of LSE + "all-reduce"
        scs.append(sc)
        cposs.append(cpos)
    go = torch.tensor([grad_out], dtype=torch.float32, device=dev)
    grads = []
    for r in range(W):
        P = plans[r]
        zq = zq_all[r * Rpad:(r + 1) * Rpad]
        cb = C.coef(scs[r], lse2_all, cposs[r], P) if keep_logits else C.coef_gemm(zq, zq_all, lse2_all, cposs[r], P)
        slabs = C.dz(cb, zqt_all, P)
        grads.append(C.norm_bwd(slabs, shards[r].contiguous(), invs[r], go, P))
    return loss, grads


def emulated_xview_forward_backward(shards: Sequence[torch.Tensor], temperature: float, *, compute: str = "auto",
                                    grad_out: float = 1.0) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """Distributed cross-view InfoNCE (:mod:`parallel.infonce`) for W virtual ranks on one device:
    loss of the global batch in pair order and per-rank dL/dh_r for shards h_r = [a_r; b_r]. Every
    rank's prep writes its slot of the shared ``zq_all`` and its merge its slot of ``lse2_all``."""
    from .infonce import _CDT, xview_compute, xview_stage_forward

    C = _ext.load()
    W = len(shards)
    R, d = shards[0].shape
    dev = shards[0].device
    comp = xview_compute(shards[0].dtype, False, compute)
    plans = [C.get_plan(R, d, W, r, float(temperature), comp, dev.index) for r in range(W)]
    Rpad = plans[0].rows_pad
    hs = [x.contiguous() for x in shards]
    zq_all = torch.empty((W * Rpad, plans[0].ld_k), dtype=_CDT[comp], device=dev)
    preps = [C.prep(hs[r], plans[r], zq_all[r * Rpad:(r + 1) * Rpad], None) for r in range(W)]  # "all-gather"
    lse2_all = torch.empty((W * Rpad,), dtype=torch.float32, device=dev)
    loss = torch.zeros((), dtype=torch.float64, device=dev)
    cposs = []
    for r in range(W):
        share, cpos = xview_stage_forward(C, plans[r], zq_all, preps[r][2], lse2_all)
        loss = loss + share  # "all-reduce" (fp64 shares)
        cposs.append(cpos)
    go = torch.tensor([grad_out], dtype=torch.float32, device=dev)
    return loss.float(), [C.xview_dist_backward(hs[r], zq_all, preps[r][1], lse2_all, cposs[r], go, plans[r]) for r in range(W)]


def emulated_sigmoid_forward_backward(shards: Sequence[torch.Tensor], temperature: float, bias: float, *,
                                      compute: str = "auto", grad_out: float = 1.0, want_tau: bool = True,
                                      want_bias: bool = True, exchange: str = "gather"):
    """Distributed pairwise sigmoid loss (:mod:`parallel.sigmoid`) for W virtual ranks on one device:
    ``(loss, grads, dtau, dbias)`` for shards h_r = [a_r; b_r]: the loss of the global batch in pair
    order, per-rank dL/dh_r, and the two scalar gradients (0-d fp32), all times ``grad_out``. Every
    rank's prep writes its slot of the shared ``zq_all``; the fp64 shares of the loss and of the
    scalar gradients are summed as the all-reduces would and rounded to fp32 once. A scalar gradient
    that is not wanted is None (with neither the backward stage returns no shares, as a backward
    that does not communicate). ``exchange="ring"`` drives the ring stage ops instead: every rank's
    prep writes a buffer of its own, and a rank's ``visit`` hands it the other virtual ranks' ``zq`` in
    ring order, q = r, r-1, ..., r-W+1, without copying."""
    from .infonce import _CDT, xview_compute
    from .sigmoid import (_check_exchange, sigmoid_ring_stage_backward, sigmoid_ring_stage_forward,
                          sigmoid_stage_forward)

    _check_exchange(exchange, "emulated_sigmoid_forward_backward")
    C = _ext.load()
    W = len(shards)
    R, d = shards[0].shape
    dev = shards[0].device
    comp = xview_compute(shards[0].dtype, False, compute)
    plans = [C.get_plan(R, d, W, r, float(temperature), comp, dev.index) for r in range(W)]
    Rpad = plans[0].rows_pad
    hs = [x.contiguous() for x in shards]
    go = torch.tensor([grad_out], dtype=torch.float32, device=dev)
    bias, wants = float(bias), (bool(want_tau), bool(want_bias))
    if exchange == "ring":
        preps = [C.prep(hs[r], plans[r]) for r in range(W)]
        zqs = [p[0] for p in preps]

        def visit_of(r):
            def visit(fn):
                for s in range(W):
                    fn((r - s) % W, zqs[(r - s) % W], 0)
            return visit

        def forward(r):
            return sigmoid_ring_stage_forward(C, plans[r], zqs[r], hs[r], preps[r][1], bias, visit_of(r))

        def backward(r):
            return sigmoid_ring_stage_backward(C, plans[r], zqs[r], hs[r], preps[r][1], bias, go, *wants, visit_of(r))
    else:
        zq_all = torch.empty((W * Rpad, plans[0].ld_k), dtype=_CDT[comp], device=dev)
        preps = [C.prep(hs[r], plans[r], zq_all[r * Rpad:(r + 1) * Rpad], None) for r in range(W)]  # "all-gather"

        def forward(r):
            return sigmoid_stage_forward(C, plans[r], zq_all, hs[r], preps[r][1], bias)

        def backward(r):
            return C.xview_sigmoid_dist_backward(hs[r], zq_all, preps[r][1], go, plans[r], bias, *wants)

    loss = torch.zeros((), dtype=torch.float64, device=dev)
    for r in range(W):
        loss = loss + forward(r)  # "all-reduce" (fp64 shares)
    grads, scalars = [], torch.zeros((2,), dtype=torch.float64, device=dev)
    for r in range(W):
        dh, shares = backward(r)
        grads.append(dh)
        if shares is not None:
            scalars = scalars + shares  # "all-reduce" (fp64 shares)
    scalars = scalars.float()
    return loss.float(), grads, scalars[0] if want_tau else None, scalars[1] if want_bias else None


def emulated_ring_forward_backward(shards: Sequence[torch.Tensor], temperature: float, *, compute: str = "auto",
                                   grad_out: float = 1.0) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """The ring-negatives stage ops (:mod:`parallel.ring`) for W virtual ranks on one device:
    every rank r visits the column blocks q = r, r-1, ... with rank q's rows as the chunk."""
    from .ring import block_tiles

    C = _ext.load()
    W = len(shards)
    R, d = shards[0].shape
    dev = shards[0].device
    comp = resolve_compute(shards[0].dtype, False, compute)
    plans = [C.get_plan(R, d, W, r, float(temperature), comp, dev.index) for r in range(W)]
    Rpad, rt = plans[0].rows_pad, plans[0].row_tiles
    preps = [C.prep(shards[r].contiguous(), plans[r]) for r in range(W)]
    zqs = [p[0] for p in preps]
    lse2_all = torch.empty((W * Rpad,), dtype=torch.float32, device=dev)
    loss = torch.zeros((), dtype=torch.float32, device=dev)
    cposs = []
    for r in range(W):
        P = plans[r]
        tiles = block_tiles(C, P, dev)
        part = torch.empty((P.col_tiles, Rpad, 2), dtype=torch.float32, device=dev)
        for s in range(W):
            q = (r - s) % W
            C.fwd_stats_tiles(zqs[r], zqs[q], q * rt, tiles[q], P, part)
        cpos = torch.empty((Rpad,), dtype=torch.float32, device=dev)
        loss = loss + C.lse(part, preps[r][2], lse2_all, cpos, P)
        cposs.append(cpos)
    go = torch.tensor([grad_out], dtype=torch.float32, device=dev)
    grads = []
    for r in range(W):
        P = plans[r]
        tiles = block_tiles(C, P, dev)
        acc = None
        for s in range(W):
            q = (r - s) % W
            cb = C.coef_gemm_tiles(zqs[r], zqs[q], q * rt, tiles[q], lse2_all, cposs[r], P, rt, q * rt)
            slabs = C.dz_block(cb, C.transpose(zqs[q], P), P)
            acc = slabs if acc is None else acc + slabs
        grads.append(C.norm_bwd(acc, shards[r].contiguous(), preps[r][1], go, P))
    return loss, grads


def emulated_sym_forward_backward(shards: Sequence[torch.Tensor], temperature: float, *, compute: str = "auto",
                                  grad_out: float = 1.0) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """The symmetric data-parallel step (csrc/runtime/sym_step.cpp, as :mod:`parallel.symmetric`
    drives it) for W virtual ranks on one device: each rank computes only its assigned cross
    blocks; the point-to-point exchanges of the plan (column partials, partner gradient
    contributions) become copies, and the rows need none (every rank writes its own slot)."""
    from .symmetric import (TILE, sym_contrib_views, sym_forward_bufs, sym_grad_slabs, sym_lse, sym_norm_bwd,
                            sym_partner_contribs, sym_step)

    C = _ext.load()
    W = len(shards)
    R, d = shards[0].shape
    dev = shards[0].device
    comp = resolve_compute(shards[0].dtype, False, compute)
    plans = [C.get_plan(R, d, W, r, float(temperature), comp, dev.index) for r in range(W)]
    steps = [sym_step(C, P, dev) for P in plans]
    P0 = plans[0]
    Rpad = P0.rows_pad
    f8 = P0.compute_dtype == "fp8"
    cdt = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[P0.backward_dtype]
    zq_all = torch.empty((W * Rpad, P0.ld_k), dtype=cdt, device=dev)
    zqt_all = torch.empty((W, P0.dim_n, P0.ld_t), dtype=cdt, device=dev)
    zq8_all = torch.empty((W * Rpad, P0.ld_k8), dtype=torch.uint8, device=dev) if f8 else None
    hs = [x.contiguous() for x in shards]
    Bs = [sym_forward_bufs(sp, P, h, zq_all, zqt_all, zq8_all) for (_, sp), P, h in zip(steps, plans, hs)]
    for (S, _), P, B in zip(steps, plans, Bs):
        S.prep(P, B)
    for (S, sp), P, B in zip(steps, plans, Bs):  # every tile in one launch: all rows are there
        S.fwd_tiles_range(P, B, 0, sp["n_fwd"])
    for r, (_, sp) in enumerate(steps):  # "send" column partials to their owners
        for (send, q, s0, s1, t0, t1, _) in sp["col_partials"]:
            if send:
                (_, _, d0, d1, _, _, _), = [x for x in steps[q][1]["col_partials"] if not x[0] and x[1] == r]
                Bs[q]["part"][d0:d1, t0 * TILE:t1 * TILE].copy_(Bs[r]["part_x"][s0:s1, t0 * TILE:t1 * TILE])
    lse2_all = torch.empty((W * Rpad,), dtype=torch.float32, device=dev)
    loss = torch.zeros((), dtype=torch.float32, device=dev)
    for (S, _), P, B in zip(steps, plans, Bs):
        loss = loss + sym_lse(S, P, B, lse2_all)  # "all-gather" of LSE + "all-reduce"
    go = torch.tensor([grad_out], dtype=torch.float32, device=dev)
    sent = []
    for (S, sp), P, B in zip(steps, plans, Bs):
        sends, _ = sym_contrib_views(sp, sym_partner_contribs(S, sp, P, B), None)
        sent.append({q: rows for rows, q in sends})
    grads = []
    for r, ((S, sp), P, B) in enumerate(zip(steps, plans, Bs)):
        B["own"], recv = sym_grad_slabs(sp, P, dev)
        S.own_grads(P, B)
        for view, p in sym_contrib_views(sp, None, recv)[1]:  # "receive"
            view.copy_(sent[p][r])
        grads.append(sym_norm_bwd(S, P, B["own"], recv, hs[r], B["inv"], go))
    return loss, grads

