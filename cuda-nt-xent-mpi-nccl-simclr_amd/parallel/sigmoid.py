"""Pairwise sigmoid loss (the SigLIP form) with the negatives of the whole data-parallel batch.

Rank r of W holds ``h_r = [a_r; b_r]`` (n rows per tower). With ``[a; b]`` the global batch in pair
order (``reference.global_pair_order``), N = W n pairs and ``x_ij = a_i . b_j / tau + bias``::

    loss = (1 / N) sum_{i,j < N} softplus(-s_ij x_ij),    s_ii = +1, s_ij = -1 otherwise

is ``reference.sigmoid_loss`` of the global batch, identical on every rank. ``dh`` is its exact
gradient w.r.t. this rank's rows (the convention of ``dist_info_nce_loss``: a trainer under DDP
multiplies by the world size); dL/dtau and dL/dbias are the exact gradients of the returned global
loss, all-reduced and identical on every rank. Temperature and bias must be the same numbers on
every rank (not checked).

* forward: prep -> all-gather of the unit rows ``zq`` (compute dtype) into ``zq_all [W Rpad][ld_k]``
  while the tiles of the own column block run -> the other blocks -> the rank's fp64 share of the
  loss -> all-reduce (8 B). Only ``a_r`` against ``b`` of all ranks is computed, an n x N block:
  every global pair is a binary term of its own and is computed exactly once somewhere, half the
  similarity FLOPs of ``dist_info_nce_loss``'s forward, and no normaliser crosses ranks.
* backward: rank-local from the saved ``h``, ``zq_all`` and ``inv``. Per side the coefficient block
  ``C = 2 G`` (``G = sigmoid(x)``, on the positives ``-sigmoid(-x)``) and its dZ rows; side 1 swaps
  the operand roles and so gives the rows of ``C^T`` directly. If a scalar gradient is wanted, one
  all-reduce of the two fp64 shares (16 B) ends it; otherwise the backward does not communicate.
  ``dh`` is bitwise the same either way.

Bytes across ranks per step and rank: the gather of ``(W - 1) Rpad ld_k`` elements of the compute
dtype, 8 B for the loss, 16 B for the scalar gradients.

``exchange="ring"`` (``RingSigmoidFunction``) holds no buffer of W slots. Every pair is a binary term of
its own, so nothing has to be agreed between ranks and a rank never needs more than one other rank's
rows at a time: rank r works on the slots q = r, r-1, ..., r-W+1 while the next one travels
(``ring._ring``), in the forward and again in the backward. Per rank: the own ``zq [Rpad][ld_k]`` (the
only unit rows saved), two ring buffers of that size, one coefficient block ``[planes][n_pad][n_pad]``,
one ``zt [2][En][n_pad]``, the fp32 dZ slab (stored by the first block, added to by the later ones) and
the tiles' partials ``lpart`` / ``bias_part`` (``nT W nT`` entries, at the gather launches' places:
the loss share and the dL/dbias share are bitwise the gather path's). Both sides are still computed
locally and no gradient crosses ranks. Bytes across ranks per step and rank: ``2 (W - 1) Rpad ld_k``
elements, twice the gather's, and the same 8 B and 16 B.

``csrc/kernels/xview_kernels.hip`` (the ``xview_sigmoid_*`` kernels); the stage ops are shared with
``parallel/emulate.emulated_sigmoid_forward_backward``.
"""
from __future__ import annotations

import contextlib
from typing import Optional

import torch
import torch.distributed as dist

from ..ops import _ext, reference
from ..ops.ntxent import _stack_views, _tau_grad, _tau_like, _TemperatureModule
from ..ops.sigmoid import _scalar_args, sigmoid_loss
from .commstats import span
from .distributed import _world
from .infonce import _gather, _gather_prologue, xview_compute
from .ring import _ring

EXCHANGES = ("gather", "ring")


def _check_exchange(exchange: str, who: str) -> None:
    if exchange not in EXCHANGES:
        raise ValueError(f"{who}: exchange must be one of {EXCHANGES}, got {exchange!r}")


def _scalar_grads(shares: Optional[torch.Tensor], tau_like, bias_like, world: int, group):
    """``(dtau, dbias)`` of the global loss from this rank's fp64 shares ``[2]``: their sum over the
    ranks (16 B), on the GPU paths rounded to fp32 once each, as ``_tau_like`` kept the two tensors. A
    like of None: that gradient is not wanted, and None is returned for it; with neither nothing is
    communicated."""
    if tau_like is None and bias_like is None:
        return None, None
    if world > 1:
        with span("sigmoid_scalars") if shares.is_cuda else contextlib.nullcontext():
            dist.all_reduce(shares, op=dist.ReduceOp.SUM, group=group)
    if shares.is_cuda:
        shares = shares.float()
    return (None if tau_like is None else _tau_grad(shares[0], tau_like),
            None if bias_like is None else _tau_grad(shares[1], bias_like))


def sigmoid_stage_forward(C, plan, zq_all: torch.Tensor, h: torch.Tensor, inv: torch.Tensor, bias: float, wait=None):
    """One rank's forward stage ops over the gathered rows: the own column block, ``wait()`` (the rows
    of the other ranks have arrived), the other blocks, the fixed-order sum. Every tile writes its own
    place of one array, so the split over two launches does not change the sum. Returns the rank's
    share of the loss, a 0-d float64 tensor."""
    W, r = plan.world, plan.rank
    lpart = torch.empty((C.xview_sigmoid_dist_tiles(plan),), dtype=torch.float64, device=zq_all.device)
    C.xview_sigmoid_dist_fwd(zq_all, plan, lpart, h, inv, bias, r, r + 1)
    if wait is not None:
        wait()
    C.xview_sigmoid_dist_fwd(zq_all, plan, lpart, h, inv, bias, 0, W, r)
    return C.xview_sigmoid_dist_loss(lpart, plan)


class DistSigmoidFunction(torch.autograd.Function):
    """``tau`` / ``bias_t`` are None, or the one-element temperature / bias tensors whose gradients
    are wanted (``ops.sigmoid.SigmoidFunction``'s convention)."""

    @staticmethod
    def forward(ctx, h: torch.Tensor, temperature: float, bias: float, compute: str, group, overlap: bool,
                tau: Optional[torch.Tensor] = None, bias_t: Optional[torch.Tensor] = None):
        C = _ext.load()
        h = h.contiguous()
        plan, zq_all, (_, inv, _, _), wait = _gather_prologue(C, h, temperature, compute, group, overlap)
        share = sigmoid_stage_forward(C, plan, zq_all, h, inv, float(bias), wait)
        if plan.world > 1:
            with span("sigmoid_loss"):
                dist.all_reduce(share, op=dist.ReduceOp.SUM, group=group)  # fp64 shares (8 B)
        ctx.plan, ctx.bias, ctx.group = plan, float(bias), group
        ctx.tau = _tau_like(tau)
        ctx.bias_like = _tau_like(bias_t)
        ctx.save_for_backward(h, zq_all, inv)
        return share.float()  # the one rounding to fp32, as the one-GPU loss has

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        h, zq_all, inv = ctx.saved_tensors
        tau = ctx.tau if ctx.needs_input_grad[6] else None
        bias_like = ctx.bias_like if ctx.needs_input_grad[7] else None
        dh, shares = _ext.load().xview_sigmoid_dist_backward(h, zq_all, inv, grad_out.reshape(1), ctx.plan, ctx.bias,
                                                             tau is not None, bias_like is not None)
        return dh, None, None, None, None, None, *_scalar_grads(shares, tau, bias_like, ctx.plan.world, ctx.group)


# ---------------------------------------------------------------------------------------
# exchange="ring": one rank slot at a time, O(local) memory
# ---------------------------------------------------------------------------------------
def sigmoid_ring_stage_forward(C, plan, zq: torch.Tensor, h: torch.Tensor, inv: torch.Tensor, bias: float, visit):
    """One rank's forward over the blocks ``visit`` hands it. ``visit(fn)`` is the transport: it calls
    ``fn(q, rows_q, ...)`` once per rank slot q in ring order (q = r, r-1, ..., r-W+1), ``rows_q
    [Rpad][ld_k]`` holding rank q's unit rows (the own block: ``zq`` itself). Every tile writes the
    place of ``lpart`` the gather launches give it, so the share is bitwise ``sigmoid_stage_forward``'s.
    Returns the rank's share of the loss, a 0-d float64 tensor."""
    lpart = torch.empty((C.xview_sigmoid_dist_tiles(plan),), dtype=torch.float64, device=zq.device)
    visit(lambda q, rows_q, *_: C.xview_sigmoid_block_fwd(zq, rows_q, q, plan, lpart, h, inv, bias))
    return C.xview_sigmoid_dist_loss(lpart, plan)


def sigmoid_ring_stage_backward(C, plan, zq: torch.Tensor, h: torch.Tensor, inv: torch.Tensor, bias: float,
                                grad_out: torch.Tensor, want_tau: bool, want_bias: bool, visit):
    """One rank's backward over the same blocks: per block the transpose, and per side the coefficient
    block ``[planes][n_pad][n_pad]`` and its dZ rows, stored by the first block and added by the later
    ones (stream-ordered, no atomics). One ``coef``, one ``zt`` and the fp32 slab serve every block; only
    ``bias_part`` (``nT * W * nT * 4`` floats) grows with W. Returns ``(dh, shares)`` as
    ``xview_sigmoid_dist_backward`` does; the dL/dbias share is bitwise its own, ``dh`` and the dL/dtau
    share are sums in block order, not slot order."""
    size = C.xview_sigmoid_block_sizes(plan)
    dev = zq.device
    coef = torch.empty((size["coef_bytes"],), dtype=torch.uint8, device=dev)
    zt = torch.empty((size["zt_bytes"],), dtype=torch.uint8, device=dev)
    bias_part = torch.empty((size["bias_part"],), dtype=torch.float32, device=dev)
    dz = torch.empty((size["dz"],), dtype=torch.float32, device=dev)
    pos = C.xview_sigmoid_pos_cos(h, inv, plan)
    first = [True]

    def block(q, rows_q, *_):
        C.xview_sigmoid_block_backward(zq, rows_q, q, plan, bias, coef, zt, bias_part, dz, pos, first[0])
        first[0] = False

    visit(block)
    del coef, zt
    return C.xview_sigmoid_ring_finish(h, inv, grad_out, dz, bias_part, plan, want_tau, want_bias)


class RingSigmoidFunction(torch.autograd.Function):
    """``DistSigmoidFunction`` with the rows passed around the ring (``ring._ring``) in both directions
    of the step: only ``h``, the own ``zq`` and ``inv`` are saved."""

    @staticmethod
    def forward(ctx, h: torch.Tensor, temperature: float, bias: float, compute: str, group,
                tau: Optional[torch.Tensor] = None, bias_t: Optional[torch.Tensor] = None):
        C = _ext.load()
        W, r = _world(group)
        h = h.contiguous()
        R, d = h.shape
        plan = C.get_plan(R, d, W, r, float(temperature), compute, h.device.index)
        # whole slots travel: prep zero-fills the K padding and the pad rows, so every row a tile stage
        # can read from a ring buffer has been received
        zq, inv, _, _ = C.prep(h, plan)
        share = sigmoid_ring_stage_forward(C, plan, zq, h, inv, float(bias), lambda fn: _ring(zq, group, fn))
        if W > 1:
            with span("sigmoid_loss"):
                dist.all_reduce(share, op=dist.ReduceOp.SUM, group=group)  # fp64 shares (8 B)
        ctx.plan, ctx.bias, ctx.group = plan, float(bias), group
        ctx.tau = _tau_like(tau)
        ctx.bias_like = _tau_like(bias_t)
        ctx.save_for_backward(h, zq, inv)
        return share.float()

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        h, zq, inv = ctx.saved_tensors
        tau = ctx.tau if ctx.needs_input_grad[5] else None
        bias_like = ctx.bias_like if ctx.needs_input_grad[6] else None
        dh, shares = sigmoid_ring_stage_backward(_ext.load(), ctx.plan, zq, h, inv, ctx.bias, grad_out.reshape(1),
                                                 tau is not None, bias_like is not None,
                                                 lambda fn: _ring(zq, ctx.group, fn))
        return dh, None, None, None, None, *_scalar_grads(shares, tau, bias_like, ctx.plan.world, ctx.group)


def dist_sigmoid_loss(h_local: torch.Tensor, temperature=0.1, bias=-10.0, *, z2: Optional[torch.Tensor] = None,
                      group=None, compute: str = "auto", use_mixed_precision: bool = False,
                      overlap: bool = True, exchange: str = "gather") -> torch.Tensor:
    """Global pairwise sigmoid loss over the data-parallel group; ``h_local = [a_r; b_r]`` on each
    rank (or ``h_local = a_r, z2 = b_r``), the same n and d on every rank.

    temperature, bias: floats or one-element tensors, the same numbers on every rank (not checked). A
      tensor that requires grad (or has a ``grad_fn``) receives the gradient of the returned global
      loss, all-reduced: identical on every rank, in the tensor's own dtype, shape and device. Loss
      and dh are bitwise those of the same floats.
    compute: ``auto|fp32|fp16|bf16|fp8`` as for ``sigmoid_loss`` (``fp8`` computes in fp16).
    overlap: launch the tiles of the own column block before the row gather is waited for (the same
      bits either way). Ignored by ``exchange="ring"``, whose every block but the last runs while the
      next one travels.
    exchange: ``"gather"`` (the default) all-gathers the unit rows once and keeps them for the
      backward; ``"ring"`` passes one rank's rows around the ring at a time, in the forward and again
      in the backward, and holds nothing whose size grows with the world size but the tiles' partial
      sums: the same loss (bitwise) and dL/dbias (bitwise before the all-reduce), ``dh`` and dL/dtau
      summed in block order. Anything else raises ``ValueError``.
    Without a process group, or in a group of one, this is ``sigmoid_loss``. CPU tensors take
    ``cpu_dist_sigmoid_loss``.
    """
    _check_exchange(exchange, "dist_sigmoid_loss")
    W, _ = _world(group)
    if W == 1:
        return sigmoid_loss(h_local, temperature, bias, z2=z2, compute=compute, use_mixed_precision=use_mixed_precision)
    h = _stack_views(h_local, z2)
    if not h.is_cuda:
        return cpu_dist_sigmoid_loss(h, temperature, bias, group=group, exchange=exchange)
    comp = xview_compute(h.dtype, use_mixed_precision, compute)
    tv, bv, tau, bias_t = _scalar_args(temperature, bias)
    if exchange == "ring":
        return RingSigmoidFunction.apply(h, tv, bv, comp, group, tau, bias_t)
    return DistSigmoidFunction.apply(h, tv, bv, comp, group, bool(overlap), tau, bias_t)


class DistSigmoidLoss(_TemperatureModule):
    """``nn.Module`` front end: ``DistSigmoidLoss(temperature, bias)(z1, z2)`` or ``(h)`` on every rank.

    ``learnable_temperature`` / ``temperature_bounds`` / ``learnable_bias`` as ``SigmoidLoss``. The
    parameters' gradients are those of the global loss, the same on every rank: they need no further
    reduction (and, under a trainer that scales the loss by the world size for DDP's mean, are
    scaled with it). ``exchange``: ``"gather"`` or ``"ring"``, as ``dist_sigmoid_loss``'s (``overlap`` is
    ignored by the ring)."""

    def __init__(self, temperature: float = 0.1, bias: float = -10.0, compute: str = "auto", group=None,
                 use_mixed_precision: bool = False, overlap: bool = True, learnable_temperature: bool = False,
                 temperature_bounds=(0.01, 1.0), learnable_bias: bool = False, exchange: str = "gather"):
        super().__init__()
        _check_exchange(exchange, "DistSigmoidLoss")
        self.exchange = exchange
        self.compute = compute
        self.group = group
        self.use_mixed_precision = use_mixed_precision
        self.overlap = overlap
        self._init_temperature(temperature, learnable_temperature, temperature_bounds)
        self.learnable_bias = bool(learnable_bias)
        self.initial_bias = float(bias)
        if self.learnable_bias:
            self.bias = torch.nn.Parameter(torch.tensor(float(bias), dtype=torch.float32))
        else:
            self.bias = float(bias)

    def forward(self, z1: torch.Tensor, z2: Optional[torch.Tensor] = None) -> torch.Tensor:
        return dist_sigmoid_loss(z1, self.current_temperature(), self.bias, z2=z2, group=self.group,
                                 compute=self.compute, use_mixed_precision=self.use_mixed_precision,
                                 overlap=self.overlap, exchange=self.exchange)

    def extra_repr(self) -> str:
        return (f"temperature={self.temperature}, bias={self.initial_bias}, compute={self.compute}"
                + self._temperature_repr() + (", learnable_bias=True" if self.learnable_bias else "")
                + (f", exchange={self.exchange}" if self.exchange != "gather" else ""))


# ---------------------------------------------------------------------------------------
# CPU / gloo path: the same algorithm (gather unit rows, side 0's n x N block forward, rank-local
# backward from both sides, one all-reduce of the two scalar shares) written with torch ops.
# ---------------------------------------------------------------------------------------
def _cpu_backward_end(ctx, z, inv, dz, g, sum_g_cos, sum_g):
    """What the two CPU backwards end with: the scale g / (N tau), the normalisation backward, and
    from side 0's sums of ``G cos`` and of ``G`` (each pair counts once) this rank's shares of the scalar
    gradients."""
    temperature, _, W, _, group, tau_like, bias_like = ctx.meta
    N = W * (z.shape[0] // 2)
    dz = dz * (g / (N * temperature))
    dot = (z * dz).sum(1, keepdim=True)
    dh = inv.unsqueeze(1) * (dz - z * dot)
    shares = torch.stack([-sum_g_cos / (N * temperature * temperature), sum_g / N]).double() * g.double()
    return (dh, None, None, None, *_scalar_grads(shares, tau_like if ctx.needs_input_grad[4] else None,
                                                 bias_like if ctx.needs_input_grad[5] else None, W, group))


class _CpuDistSigmoidFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, temperature, bias, group, tau, bias_t):
        W, r = _world(group)
        n = h.shape[0] // 2
        z, inv = reference.normalize(h)
        zs = _gather(z, W, group)
        # towers[v]: view v of every rank, rank slots in order (the columns of side 1 - v)
        towers = [torch.cat([q[:n] for q in zs], 0), torch.cat([q[n:] for q in zs], 0)]
        x = z[:n] @ towers[1].t() / temperature + bias  # side 0 only: every global pair once
        s = -torch.ones_like(x)
        s[torch.arange(n), torch.arange(n) + r * n] = 1.0
        loss = torch.nn.functional.softplus(-s * x).sum() / (W * n)
        if W > 1:
            dist.all_reduce(loss, group=group)
        ctx.save_for_backward(z, inv, *towers)
        ctx.meta = (temperature, bias, W, r, group, _tau_like(tau), _tau_like(bias_t))
        return loss

    @staticmethod
    def backward(ctx, g):
        z, inv, t0, t1 = ctx.saved_tensors
        temperature, bias, _, r, _, _, _ = ctx.meta
        n = z.shape[0] // 2
        ar = torch.arange(n)
        towers = (t0, t1)
        dz, G0 = [], None
        for v in (0, 1):  # side 1: the same formula with the roles swapped gives the rows of G^T
            cos = z[v * n:(v + 1) * n] @ towers[1 - v].t()
            x = cos / temperature + bias
            G = torch.sigmoid(x)
            G[ar, ar + r * n] = -torch.sigmoid(-x[ar, ar + r * n])
            dz.append(G @ towers[1 - v])
            if v == 0:
                G0, cos0 = G, cos
        return _cpu_backward_end(ctx, z, inv, torch.cat(dz, 0), g, (G0 * cos0).sum(), G0.sum())


class _CpuRingSigmoidFn(torch.autograd.Function):
    """The ring variant: the unit rows of one rank at a time over gloo send / recv (``ring._ring``), in the
    block order q = r, r-1, ..., r-W+1 of the GPU path, forward and backward; the towers are never
    concatenated, and only ``z`` and ``inv`` are saved."""

    @staticmethod
    def forward(ctx, h, temperature, bias, group, tau, bias_t):
        W, r = _world(group)
        n = h.shape[0] // 2
        z, inv = reference.normalize(h)
        ar = torch.arange(n)
        total = [torch.zeros((), dtype=z.dtype)]

        def block(q, zq, *_):  # side 0 only: every global pair once
            x = z[:n] @ zq[n:].t() / temperature + bias
            s = -torch.ones_like(x)
            if q == r:
                s[ar, ar] = 1.0
            total[0] = total[0] + torch.nn.functional.softplus(-s * x).sum()

        _ring(z, group, block)
        loss = total[0] / (W * n)
        if W > 1:
            dist.all_reduce(loss, group=group)
        ctx.save_for_backward(z, inv)
        ctx.meta = (temperature, bias, W, r, group, _tau_like(tau), _tau_like(bias_t))
        return loss

    @staticmethod
    def backward(ctx, g):
        z, inv = ctx.saved_tensors
        temperature, bias, _, r, group, _, _ = ctx.meta
        n = z.shape[0] // 2
        ar = torch.arange(n)
        dz = torch.zeros_like(z)
        sums = torch.zeros(2, dtype=z.dtype)  # side 0's sum of G cos and of G: each pair counts once

        def block(q, zq, *_):
            for v in (0, 1):  # side 1: the same formula with the roles swapped gives the rows of G^T
                other = zq[(1 - v) * n:(2 - v) * n]
                cos = z[v * n:(v + 1) * n] @ other.t()
                x = cos / temperature + bias
                G = torch.sigmoid(x)
                if q == r:
                    G[ar, ar] = -torch.sigmoid(-x[ar, ar])
                dz[v * n:(v + 1) * n] += G @ other
                if v == 0:
                    sums[0] += (G * cos).sum()
                    sums[1] += G.sum()

        _ring(z, group, block)
        return _cpu_backward_end(ctx, z, inv, dz, g, sums[0], sums[1])


def cpu_dist_sigmoid_loss(h_local: torch.Tensor, temperature=0.1, bias=-10.0, group=None,
                          exchange: str = "gather") -> torch.Tensor:
    """The distributed algorithm in torch ops over gloo, for CPU tensors (any float dtype);
    ``exchange`` as ``dist_sigmoid_loss``'s."""
    _check_exchange(exchange, "cpu_dist_sigmoid_loss")
    fn = _CpuRingSigmoidFn if exchange == "ring" else _CpuDistSigmoidFn
    tv, bv, tau, bias_t = _scalar_args(temperature, bias)
    return fn.apply(_stack_views(h_local, None), tv, bv, group, tau, bias_t)
