"""Cross-view InfoNCE (the CLIP form) with the negatives of the whole data-parallel batch.

Rank r of W holds ``h_r = [a_r; b_r]`` (n rows per tower). The loss is ``reference.info_nce_loss`` of
the global batch in pair order, ``[a_0; ..; a_{W-1}; b_0; ..; b_{W-1}]`` (N = W n pairs), identical
on every rank, and the gradient is its exact gradient w.r.t. this rank's rows (the convention of
``dist_ntxent_loss``: a trainer under DDP multiplies by the world size).

* forward: prep -> all-gather of the unit rows ``zq`` (compute dtype) into ``zq_all [W Rpad][ld_k]``
  while the tiles of the own column block run -> the other blocks -> per-pair merge -> all-gather of
  ``lse2`` (Rpad floats per rank) + all-reduce of the loss (4 B). Per side v the rows are view v of this
  rank and the columns view 1 - v of all ranks: both n x N blocks are computed here, twice the
  similarity FLOPs of a scheme that exchanges column partials, and in return nothing else crosses ranks.
* backward: rank-local. ``G_ij = P_ij + P_ji - 2 [j = p(i)]`` needs only the gathered LSE; side 1 is
  the same formula with the operand roles swapped, which yields the rows of ``G^T`` directly. The
  transposed operand of the dZ products is made locally from the gathered rows.

``csrc/kernels/xview_kernels.hip`` (the ``xview_dist_*`` kernels); the stage ops are shared with
``parallel/emulate.emulated_xview_forward_backward``.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist

from ..ops import _ext, reference
from ..ops.infonce import info_nce_loss
from ..ops.ntxent import _stack_views, refuse_temperature_grad, resolve_compute, temperature_value
from .commstats import span
from .distributed import _all_gather_into, _world

_CDT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def xview_compute(dtype: torch.dtype, use_mixed_precision: bool, compute: str) -> str:
    """The compute dtype of the cross-view kernels: ``resolve_compute``, with fp8 computed in fp16."""
    comp = resolve_compute(dtype, use_mixed_precision, compute)
    return "fp16" if comp == "fp8" else comp


def xview_stage_forward(C, plan, zq_all: torch.Tensor, ypos: torch.Tensor, lse2_all: torch.Tensor, wait=None):
    """One rank's forward stage ops over the gathered rows: the own column block, ``wait()`` (the rows
    of the other ranks have arrived), the other blocks, the merge into this rank's slot of
    ``lse2_all``. Returns (loss share, a 0-d float64 tensor; cpos)."""
    W, r, Rpad = plan.world, plan.rank, plan.rows_pad
    part = torch.empty((C.xview_dist_part_slots(plan), Rpad, 2), dtype=torch.float32, device=zq_all.device)
    C.xview_dist_fwd(zq_all, plan, part, ypos, r, r + 1)
    if wait is not None:
        wait()
    C.xview_dist_fwd(zq_all, plan, part, ypos, 0, W, r)
    cpos = torch.empty((Rpad,), dtype=torch.float32, device=zq_all.device)
    return C.xview_dist_lse(part, ypos, lse2_all, cpos, plan), cpos


def _gather_prologue(C, h: torch.Tensor, temperature: float, compute: str, group, overlap: bool):
    """What the gather Functions' forwards open with: this rank's plan, ``prep`` of the contiguous ``h``
    straight into its slot of ``zq_all [W Rpad][ld_k]`` and the all-gather of the slots, started there:
    the gather runs in place. Returns ``(plan, zq_all, prep's outputs, wait)``. ``wait`` is for the
    stage forward: it makes the stream wait for the rows of the other ranks, or is None if they need
    no waiting for (without ``overlap`` that is done here)."""
    W, r = _world(group)
    R, d = h.shape
    plan = C.get_plan(R, d, W, r, float(temperature), compute, h.device.index)
    Rpad = plan.rows_pad
    zq_all = torch.empty((W * Rpad, plan.ld_k), dtype=_CDT[compute], device=h.device)
    zq = zq_all[r * Rpad:(r + 1) * Rpad]
    st = C.prep(h, plan, zq, None)
    work = _all_gather_into(zq_all, zq, group, async_op=True) if W > 1 else None

    def wait():
        if work is not None:
            with span("fwd_rows"):
                work.wait()

    if not overlap:
        wait()
    return plan, zq_all, st, wait if overlap else None


class DistInfoNCEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h: torch.Tensor, temperature: float, compute: str, group, overlap: bool):
        C = _ext.load()
        h = h.contiguous()
        plan, zq_all, (_, inv, ypos, _), wait = _gather_prologue(C, h, temperature, compute, group, overlap)
        W, r, Rpad = plan.world, plan.rank, plan.rows_pad
        lse2_all = torch.empty((W * Rpad,), dtype=torch.float32, device=h.device)
        share, cpos = xview_stage_forward(C, plan, zq_all, ypos, lse2_all, wait)
        if W > 1:
            mine = lse2_all[r * Rpad:(r + 1) * Rpad].clone()
            with span("lse_loss"):
                _all_gather_into(lse2_all, mine, group)
                dist.all_reduce(share, op=dist.ReduceOp.SUM, group=group)  # fp64 shares (8 B)
        ctx.plan = plan
        ctx.save_for_backward(h, zq_all, inv, lse2_all, cpos)
        return share.float()  # the one rounding to fp32, as the one-GPU loss has

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        h, zq_all, inv, lse2_all, cpos = ctx.saved_tensors
        dh = _ext.load().xview_dist_backward(h, zq_all, inv, lse2_all, cpos, grad_out.reshape(1), ctx.plan)
        return dh, None, None, None, None


def dist_info_nce_loss(h_local: torch.Tensor, temperature=0.07, *, z2: Optional[torch.Tensor] = None, group=None,
                       compute: str = "auto", use_mixed_precision: bool = False, overlap: bool = True) -> torch.Tensor:
    """Global cross-view InfoNCE over the data-parallel group; ``h_local = [a_r; b_r]`` on each rank
    (or ``h_local = a_r, z2 = b_r``), the same n and d on every rank.

    compute: ``auto|fp32|fp16|bf16|fp8`` as for ``info_nce_loss`` (``fp8`` computes in fp16).
    overlap: launch the tiles of the own column block before the row gather is waited for (the same
    bits either way). A temperature that requires grad is refused, as in every distributed path.
    Without a process group, or in a group of one, this is ``info_nce_loss``. CPU tensors take
    ``cpu_dist_info_nce_loss``.
    """
    refuse_temperature_grad(temperature, "dist_info_nce_loss")
    W, _ = _world(group)
    if W == 1:
        return info_nce_loss(h_local, temperature, z2=z2, compute=compute, use_mixed_precision=use_mixed_precision)
    h = _stack_views(h_local, z2)
    if not h.is_cuda:
        return cpu_dist_info_nce_loss(h, temperature, group=group)
    comp = xview_compute(h.dtype, use_mixed_precision, compute)
    return DistInfoNCEFunction.apply(h, temperature_value(temperature), comp, group, bool(overlap))


class DistInfoNCELoss(torch.nn.Module):
    """``nn.Module`` front end: ``DistInfoNCELoss(temperature)(z1, z2)`` or ``(h)`` on every rank."""

    def __init__(self, temperature=0.07, compute: str = "auto", group=None, use_mixed_precision: bool = False,
                 overlap: bool = True):
        super().__init__()
        self.temperature = temperature
        self.compute = compute
        self.group = group
        self.use_mixed_precision = use_mixed_precision
        self.overlap = overlap

    def forward(self, z1: torch.Tensor, z2: Optional[torch.Tensor] = None) -> torch.Tensor:
        return dist_info_nce_loss(z1, self.temperature, z2=z2, group=self.group, compute=self.compute,
                                  use_mixed_precision=self.use_mixed_precision, overlap=self.overlap)

    def extra_repr(self) -> str:
        return f"temperature={temperature_value(self.temperature)}, compute={self.compute}"


# ---------------------------------------------------------------------------------------
# CPU / gloo path: the same algorithm (gather unit rows + LSE, rank-local backward from both sides)
# written with torch ops. Used for multi-process tests without GPUs.
# ---------------------------------------------------------------------------------------
def _gather(x: torch.Tensor, W: int, group):
    if W == 1:
        return [x]
    parts = [torch.empty_like(x) for _ in range(W)]
    dist.all_gather(parts, x.contiguous(), group=group)
    return parts


class _CpuDistInfoNCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, temperature, group):
        W, r = _world(group)
        n = h.shape[0] // 2
        z, inv = reference.normalize(h)
        zs = _gather(z, W, group)
        # towers[v]: view v of every rank, rank slots in order (the columns of side 1 - v)
        towers = [torch.cat([q[:n] for q in zs], 0), torch.cat([q[n:] for q in zs], 0)]
        pos = torch.arange(n) + r * n
        S = [z[v * n:(v + 1) * n] @ towers[1 - v].t() / temperature for v in (0, 1)]
        lse = torch.cat([torch.logsumexp(s, 1) for s in S])
        loss = sum((lse[v * n:(v + 1) * n] - S[v][torch.arange(n), pos]).sum() for v in (0, 1)) / (2 * W * n)
        lses = _gather(lse, W, group)
        if W > 1:
            dist.all_reduce(loss, group=group)
        lse_cols = [torch.cat([q[:n] for q in lses]), torch.cat([q[n:] for q in lses])]  # by view
        ctx.save_for_backward(z, inv, lse, *towers, *S, *lse_cols)
        ctx.meta = (temperature, W, r)
        return loss

    @staticmethod
    def backward(ctx, g):
        z, inv, lse, t0, t1, s0, s1, l0, l1 = ctx.saved_tensors
        temperature, W, r = ctx.meta
        n = z.shape[0] // 2
        ar = torch.arange(n)
        towers, S, lse_cols = (t0, t1), (s0, s1), (l0, l1)
        dz = []
        for v in (0, 1):  # G = P_ij + P_ji - 2 [j = p(i)]; side 1 gives the rows of G^T directly
            G = torch.exp(S[v] - lse[v * n:(v + 1) * n].unsqueeze(1)) + torch.exp(S[v] - lse_cols[1 - v].unsqueeze(0))
            G[ar, ar + r * n] -= 2.0
            dz.append(G @ towers[1 - v])
        dz = torch.cat(dz, 0) * (g / (2 * W * n * temperature))
        dot = (z * dz).sum(1, keepdim=True)
        return inv.unsqueeze(1) * (dz - z * dot), None, None


def cpu_dist_info_nce_loss(h_local: torch.Tensor, temperature=0.07, group=None) -> torch.Tensor:
    """The distributed algorithm in torch ops over gloo, for CPU tensors (any float dtype)."""
    refuse_temperature_grad(temperature, "cpu_dist_info_nce_loss")
    return _CpuDistInfoNCEFn.apply(_stack_views(h_local, None), temperature_value(temperature), group)
