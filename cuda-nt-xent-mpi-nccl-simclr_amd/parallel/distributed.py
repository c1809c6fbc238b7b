"""Global-batch negatives across GPUs: RCCL (``torch.distributed`` backend ``nccl``) over xGMI.

The reference only links MPI/NCCL in CMake (``CMakeLists.txt:13-14,41-47,115-121``) and never
calls them; the repo name promises a multi-GPU SimCLR loss. Design:

* rank r holds ``h_r = [h1_r; h2_r]`` (R = 2n rows). Positives are rank-local, global column
  index = r * Rpad + local row.
* forward: prep -> all-gather Zq (compute dtype, 32 MiB/rank at B=4096, d=2048) while the
  own-rank (upper-triangular) tiles run -> remote tiles -> LSE -> all-gather LSE (fp32,
  Rpad floats/rank) + all-reduce of the loss (4 B).
* the ZqT all-gather (B operand of dZ) is issued asynchronously right after prep and is only
  waited for in the backward, so it hides under the forward GEMM.
* backward is rank-local thanks to the symmetric trick: C_ij = P_ij + P_ji - 2[j=p(i)] needs
  only the gathered LSE; no reduce-scatter of column gradients.

The returned loss is the global NT-Xent over all W*R rows (identical on every rank), and the
gradient is its exact gradient w.r.t. this rank's rows.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist

from ..ops import _ext, reference
from ..ops.ntxent import refuse_temperature_grad, resolve_compute
from .commstats import comm_reserve_cus, span


def _world(group) -> tuple[int, int]:
    if not dist.is_available() or not dist.is_initialized():
        return 1, 0
    return dist.get_world_size(group), dist.get_rank(group)


def _is_gloo(group) -> bool:
    return dist.get_backend(group) == "gloo"


class _Done:
    """Completed-work stand-in for the synchronous gloo fallbacks."""

    def wait(self):
        return True


def _all_gather_into(out: torch.Tensor, inp: torch.Tensor, group, async_op: bool = False):
    """``all_gather_into_tensor`` on RCCL (in place: ``inp`` is this rank's slot of ``out``).
    gloo (the 1-GPU multi-process test backend) gathers into a list and copies."""
    if not _is_gloo(group):
        return dist.all_gather_into_tensor(out, inp, group=group, async_op=async_op)
    W = dist.get_world_size(group)
    parts = list(out.chunk(W, 0))
    src = inp.detach().to("cpu")  # gloo gathers host tensors only
    tmp = [torch.empty_like(src) for _ in parts]
    dist.all_gather(tmp, src, group=group)
    for p, t in zip(parts, tmp):
        p.copy_(t.view(p.shape), non_blocking=False)
    return _Done() if async_op else None


def _reduce_scatter_sum(out: torch.Tensor, inp: torch.Tensor, group):
    if not _is_gloo(group):
        dist.reduce_scatter_tensor(out, inp, op=dist.ReduceOp.SUM, group=group)
        return
    full = inp.clone()  # gloo has no reduce-scatter: all-reduce, keep this rank's slice
    dist.all_reduce(full, group=group)
    out.copy_(full.chunk(dist.get_world_size(group), 0)[dist.get_rank(group)])


class DistNTXentFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h: torch.Tensor, temperature: float, compute: str, group, keep_logits: bool,
                overlap: bool, backward_mode: str = "symmetric"):
        C = _ext.load()
        W, r = _world(group)
        h = h.contiguous()
        R, d = h.shape
        plan = C.get_plan(R, d, W, r, float(temperature), compute, h.device.index)
        Rpad = plan.rows_pad
        f8 = plan.compute_dtype == "fp8"
        keep_logits = keep_logits or f8  # fp8 plans always keep their (fp16) cosines
        cdt = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[plan.backward_dtype]
        # prep / transpose write straight into this rank's slot: the gathers run in place.
        zq_all = torch.empty((W * Rpad, plan.ld_k), dtype=cdt, device=h.device)
        zqt_all = torch.empty((W, plan.dim_n, plan.ld_t), dtype=cdt, device=h.device)
        zq = zq_all[r * Rpad:(r + 1) * Rpad]
        zqt = zqt_all[r]
        # fp8: the forward GEMM (and so the forward gather) uses the 1-byte e4m3 rows
        fwd_all = torch.empty((W * Rpad, plan.ld_k8), dtype=torch.uint8, device=h.device) if f8 else zq_all
        fwd = fwd_all[r * Rpad:(r + 1) * Rpad]
        _, inv, ypos, _ = C.prep(h, plan, zq, fwd if f8 else None)
        C.transpose(zq, plan, zqt)
        work_z = work_t = None
        if W > 1:
            work_z = _all_gather_into(fwd_all, fwd, group, async_op=True)
            work_t = _all_gather_into(zqt_all, zqt, group, async_op=True)
            if not overlap:
                work_z.wait()
                work_z = None
        part = torch.empty((plan.col_tiles, Rpad, 2), dtype=torch.float32, device=h.device)
        sc = torch.empty((plan.n_fwd_tiles * 256 * 256,), dtype=cdt, device=h.device) if keep_logits else None
        # own-rank (upper-triangular) tiles need only this rank's slot: they overlap the gather
        reserve = comm_reserve_cus(dist.get_backend(group)) if W > 1 else 0
        C.fwd_stats_range(fwd, fwd_all, plan, part, sc, 0, plan.n_own_tiles, reserve_cus=reserve)
        if work_z is not None:
            with span("fwd_rows"):
                work_z.wait()
        C.fwd_stats_range(fwd, fwd_all, plan, part, sc, plan.n_own_tiles, plan.n_fwd_tiles - plan.n_own_tiles,
                          reserve_cus=reserve if work_t is not None else 0)  # the ZqT gather is in flight
        lse2_all = torch.empty((W * Rpad,), dtype=torch.float32, device=h.device)
        cpos = torch.empty((Rpad,), dtype=torch.float32, device=h.device)
        loss = C.lse(part, ypos, lse2_all, cpos, plan)
        if W > 1:
            mine = lse2_all[r * Rpad:(r + 1) * Rpad].clone()
            with span("lse_loss"):
                _all_gather_into(lse2_all, mine, group)
                dist.all_reduce(loss, op=dist.ReduceOp.SUM, group=group)
        ctx.plan = plan
        ctx.group = group
        ctx.backward_mode = backward_mode
        ctx.work_t = work_t
        ctx.sc = sc if keep_logits else None
        ctx.save_for_backward(h, zq, zq_all, zqt_all, inv, lse2_all, cpos)
        return loss

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        C = _ext.load()
        h, zq, zq_all, zqt_all, inv, lse2_all, cpos = ctx.saved_tensors
        if ctx.work_t is not None:
            with span("bwd_rows"):
                ctx.work_t.wait()
            ctx.work_t = None
        sc, ctx.sc = ctx.sc, None
        if ctx.backward_mode == "reduce_scatter":
            dh = _reduce_scatter_backward(ctx.plan, h, zq, zqt_all, inv, lse2_all, grad_out, ctx.group)
            return dh, None, None, None, None, None, None
        if sc is not None:
            sc = C.coef(sc, lse2_all, cpos, ctx.plan)
        else:
            sc = C.coef_gemm(zq, zq_all, lse2_all, cpos, ctx.plan)
        slabs = C.dz(sc, zqt_all, ctx.plan)
        dh = C.norm_bwd(slabs, h, inv, grad_out.reshape(1), ctx.plan)
        return dh, None, None, None, None, None, None


def _reduce_scatter_backward(plan, h, zq, zqt_all, inv, lse2_all, grad_out, group):
    """Comparison variant named by the north star: each rank differentiates only ITS loss terms
    w.r.t. ALL gathered rows (row part locally, column part G_cols = D^T z_local for every
    global row) and a reduce-scatter sums the column parts onto their owners.

    D = P_rows - I_pos (row softmax of this rank's rows over global columns). Costs O(R * W R)
    memory and a W*R x d fp32 reduce-scatter (512 MiB at 8 x 4096 x 2048) per step, versus an
    LSE all-gather of W*R floats for the symmetric backward — which is why the symmetric
    variant is the default. torch ops + RCCL; kept for A/B comparison.
    """
    W, r = _world(group)
    R, d = h.shape
    Rpad = plan.rows_pad
    n = R // 2
    T = plan.temperature
    z = zq[:R, :d].float()
    # every rank's rows from the gathered transposes (gathered in every precision mode)
    rows_all = torch.cat([zqt_all[q, :d, :R].t() for q in range(W)], 0).float()  # [W*R, d]
    S = z @ rows_all.t() / T
    ar = torch.arange(R, device=h.device)
    S[ar, ar + r * R] = float("-inf")
    lse_nat = torch.cat([lse2_all[q * Rpad:q * Rpad + R] for q in range(W)]) * 0.6931471805599453
    D = torch.exp(S - lse_nat[r * R:(r + 1) * R].unsqueeze(1))
    D[ar, (ar + n) % R + r * R] -= 1.0
    N2 = W * R
    scale = grad_out.reshape(()).float() / (N2 * T)
    g_rows = (D @ rows_all) * scale                      # d(own terms)/d(own rows), row part
    g_cols = (D.t() @ z) * scale                         # d(own terms)/d(every row), column part
    if W > 1:
        mine = torch.empty((R, d), dtype=torch.float32, device=h.device)
        with span("bwd_reduce_scatter"):
            _reduce_scatter_sum(mine, g_cols.contiguous(), group)
    else:
        mine = g_cols
    dz = g_rows + mine
    zf = h.float() * inv.unsqueeze(1)
    dot = (zf * dz).sum(1, keepdim=True)
    return (inv.unsqueeze(1) * (dz - zf * dot)).to(h.dtype)


def dist_ntxent_loss(h_local: torch.Tensor, temperature: float = 0.07, *, group=None, compute: str = "auto",
                     use_mixed_precision: bool = False, keep_logits: bool = True, overlap: bool = True,
                     backward_mode: str = "symmetric", negatives: str = "allgather",
                     impl: str = "auto") -> torch.Tensor:
    """Global NT-Xent over the data-parallel group; ``h_local = [h1_r; h2_r]`` on each rank.

    backward_mode: ``"symmetric"`` (default: rank-local C = P + P^T - 2 I_pos from the gathered
    LSE, no gradient collective) or ``"reduce_scatter"`` (column gradients reduce-scattered to
    their owners; comparison variant).
    negatives: ``"allgather"`` (default: every rank computes its whole row block against the
    gathered rows), ``"symmetric"`` (each rank pair's similarity block computed once, column
    partials and partner gradient contributions exchanged point to point, see
    :mod:`parallel.symmetric`), or ``"ring"`` (rows passed point-to-point around the ring,
    O(local) memory, see :mod:`parallel.ring`).
    impl: ``"auto"`` (default: the native C++ engine of :mod:`parallel.engine_loss` whenever it
    can run the call -- RCCL group, GPU tensors, symmetric or all-gather negatives, symmetric
    backward, overlap on -- else the torch-driven stages), ``"engine"`` (required; raises if not
    eligible) or ``"torch"`` (the Python-driven stages over ``torch.distributed``).
    """
    refuse_temperature_grad(temperature, "dist_ntxent_loss")
    if negatives not in ("allgather", "ring", "symmetric"):
        raise ValueError("negatives must be 'allgather', 'symmetric' or 'ring'")
    if impl not in ("auto", "engine", "torch"):
        raise ValueError("impl must be 'auto', 'engine' or 'torch'")
    if impl != "torch":
        from .engine_loss import engine_eligible, engine_ntxent_loss

        ok, why = engine_eligible(h_local, group, negatives, backward_mode, overlap)
        if ok:
            comp = resolve_compute(h_local.dtype, use_mixed_precision, compute)
            return engine_ntxent_loss(h_local, temperature, group=group, compute=comp, negatives=negatives,
                                      keep_logits=keep_logits or negatives == "symmetric",
                                      comm_reserve_cus=comm_reserve_cus(dist.get_backend(group)))
        if impl == "engine":
            raise ValueError(f"dist_ntxent_loss(impl='engine'): not eligible ({why})")
    if negatives == "symmetric":
        from .symmetric import sym_ntxent_loss

        return sym_ntxent_loss(h_local, temperature, group=group, compute=compute,
                               use_mixed_precision=use_mixed_precision)
    if negatives == "ring":
        from .ring import ring_ntxent_loss

        return ring_ntxent_loss(h_local, temperature, group=group, compute=compute,
                                use_mixed_precision=use_mixed_precision)
    if backward_mode not in ("symmetric", "reduce_scatter"):
        raise ValueError("backward_mode must be 'symmetric' or 'reduce_scatter'")
    if not h_local.is_cuda:
        return cpu_dist_ntxent_loss(h_local, temperature, group=group, backward_mode=backward_mode)
    comp = resolve_compute(h_local.dtype, use_mixed_precision, compute)
    return DistNTXentFunction.apply(h_local, float(temperature), comp, group, bool(keep_logits), bool(overlap),
                                    backward_mode)


# ---------------------------------------------------------------------------------------
# CPU / gloo path: the same algorithm (gather normalised rows + LSE, rank-local symmetric
# backward) written with torch ops. Used for multi-process tests without GPUs.
# ---------------------------------------------------------------------------------------
class _CpuDistFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, temperature, group, backward_mode="symmetric"):
        W, r = _world(group)
        R = h.shape[0]
        n = R // 2
        z, inv = reference.normalize(h)
        if W > 1:
            parts = [torch.empty_like(z) for _ in range(W)]
            dist.all_gather(parts, z.contiguous(), group=group)
            z_all = torch.cat(parts, 0)
        else:
            z_all = z
        S = z @ z_all.t() / temperature
        own = torch.arange(R) + r * R
        S[torch.arange(R), own] = float("-inf")
        lse = torch.logsumexp(S, 1)
        pos = (torch.arange(R) + n) % R + r * R
        loss = (lse - S[torch.arange(R), pos]).sum() / (W * R)
        if W > 1:
            lparts = [torch.empty_like(lse) for _ in range(W)]
            dist.all_gather(lparts, lse.contiguous(), group=group)
            lse_all = torch.cat(lparts)
            dist.all_reduce(loss, group=group)
        else:
            lse_all = lse
        ctx.save_for_backward(z, inv, z_all, S, lse, lse_all)
        ctx.meta = (temperature, W, r, backward_mode, group)
        return loss

    @staticmethod
    def backward(ctx, g):
        z, inv, z_all, S, lse, lse_all = ctx.saved_tensors
        temperature, W, r, mode, group = ctx.meta
        R = z.shape[0]
        n = R // 2
        ar = torch.arange(R)
        if mode == "reduce_scatter":
            D = torch.exp(S - lse.unsqueeze(1))
            D[ar, (ar + n) % R + r * R] -= 1.0
            scale = g / (W * R * temperature)
            cols = (D.t() @ z) * scale
            if W > 1:  # gloo has no reduce_scatter: all-reduce, keep this rank's slice
                dist.all_reduce(cols, group=group)
            dz = (D @ z_all) * scale + cols[r * R:(r + 1) * R]
        else:
            Cm = torch.exp(S - lse.unsqueeze(1)) + torch.exp(S - lse_all.unsqueeze(0))
            Cm[ar, ar + r * R] = 0.0
            Cm[ar, (ar + n) % R + r * R] -= 2.0
            dz = Cm @ z_all * (g / (W * R * temperature))
        dot = (z * dz).sum(1, keepdim=True)
        return inv.unsqueeze(1) * (dz - z * dot), None, None, None


def cpu_dist_ntxent_loss(h_local: torch.Tensor, temperature: float = 0.07, group=None,
                         backward_mode: str = "symmetric") -> torch.Tensor:
    refuse_temperature_grad(temperature, "cpu_dist_ntxent_loss")
    return _CpuDistFn.apply(h_local, float(temperature), group, backward_mode)
