"""Pairwise sigmoid loss on MI355X: the SigLIP form of the two-tower loss, one GPU.

For L2-normalised towers ``A, B`` of ``N`` rows each and ``x_ij = a_i . b_j / tau + bias``::

    loss = (1 / N) sum_ij softplus(-s_ij x_ij),    s_ii = +1, s_ij = -1 (i != j)

Every one of the N x N pairs is a binary term of its own: no softmax normaliser, and a bias that is
usually learned beside the temperature (SigLIP starts from ``t = 1 / tau = 10``, ``bias = -10``). Rows
are stacked as everywhere in the package, ``h = [h1; h2]``.

Execution: prep (L2-normalise) -> in 16-bit computes the pairs' cosines from the fp32 unit rows (the
positives' logits: nothing here cancels the shift that rounding the unit rows gives them) -> MFMA
tile GEMM of the N x N block ``Z1 Z2^T`` whose epilogue sums the tile's softplus terms into one
partial -> deterministic sum; backward: prep again (and the pairs' cosines again) -> the
coefficient block ``C = 2 G`` (``G_ij = sigmoid(x_ij)``, ``G_ii = -sigmoid(-x_ii)``) written once in
InfoNCE's plane layout, with the per-wave partials of ``sum G`` for dL/dbias -> ``C Z2`` and
``C^T Z1`` on MFMA into an fp32 slab -> grad_out/(2N tau) scale + L2-normalisation backward, whose
per-row dots give dL/dtau (``csrc/kernels/xview_kernels.hip``).
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import _ext, reference
from .ntxent import (_stack_views, _tau_grad, _tau_like, _TemperatureModule, _use_reference, resolve_compute,
                     temperature_wants_grad)


def _one_element(v, name: str):
    if isinstance(v, torch.Tensor) and v.numel() != 1:
        raise ValueError(f"{name} must be a float or a one-element tensor")
    return v


def _scalar_args(temperature, bias):
    """What the sigmoid Functions take of ``(temperature, bias)``: ``(tv, bv, tau, bias_t)``, the two as
    host floats and, where autograd tracks it, the tensor whose gradient is wanted (None otherwise).
    One-element tensors are read on the host: two tensors on the same GPU together, in a single copy
    (one host sync per forward); tensors on two different GPUs cost a sync each, CPU tensors none."""
    vals = [_one_element(temperature, "temperature"), _one_element(bias, "bias")]
    dev = [i for i, v in enumerate(vals) if isinstance(v, torch.Tensor) and v.is_cuda]
    if len(dev) == 2 and vals[0].device == vals[1].device:
        host = torch.stack([vals[0].detach().reshape(()).double(), vals[1].detach().reshape(()).double()]).tolist()
    else:
        host = [float(v.detach().item()) if isinstance(v, torch.Tensor) else float(v) for v in vals]
    return (float(host[0]), float(host[1]), *(v if temperature_wants_grad(v) else None for v in vals))


class SigmoidFunction(torch.autograd.Function):
    """loss = sigmoid_loss(h) for stacked views h = [h1; h2] on one GPU.

    ``tau`` / ``bias_t`` are None, or the one-element temperature / bias tensors whose gradients are
    wanted: the backward then also returns dL/dtau / dL/dbias in those tensors' dtype, shape and
    device."""

    @staticmethod
    def forward(ctx, h: torch.Tensor, temperature: float, bias: float, compute: str,
                tau: Optional[torch.Tensor] = None, bias_t: Optional[torch.Tensor] = None):
        C = _ext.load()
        h = h.contiguous()
        loss, inv = C.xview_sigmoid_forward(h, float(temperature), float(bias), compute)
        ctx.temperature = float(temperature)
        ctx.bias = float(bias)
        ctx.compute = compute
        ctx.tau = _tau_like(tau)
        ctx.bias_like = _tau_like(bias_t)
        ctx.save_for_backward(h, inv)
        return loss

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        C = _ext.load()
        h, inv = ctx.saved_tensors
        want_tau = ctx.tau is not None and ctx.needs_input_grad[4]
        want_bias = ctx.bias_like is not None and ctx.needs_input_grad[5]
        dh, dtau, dbias = C.xview_sigmoid_backward(h, inv, grad_out.reshape(1), ctx.temperature, ctx.bias, ctx.compute,
                                                   want_tau, want_bias)
        return (dh, None, None, None, _tau_grad(dtau, ctx.tau) if want_tau else None,
                _tau_grad(dbias, ctx.bias_like) if want_bias else None)


def sigmoid_loss(h: torch.Tensor, temperature=0.1, bias=-10.0, *, z2: Optional[torch.Tensor] = None,
                 compute: str = "auto", use_mixed_precision: bool = False) -> torch.Tensor:
    """Pairwise sigmoid loss of stacked views ``h = [h1; h2]`` (or ``h1=h, z2=h2``; the two may come
    from different encoders: autograd splits the gradient).

    Args:
      temperature, bias: floats or one-element tensors. A tensor that requires grad (or has a
        ``grad_fn``, e.g. ``log_temperature.exp()``) receives its gradient from the backward, in its
        own dtype, shape and on its own device; loss and dh are bitwise those of the same floats. The
        kernels take both by value: reading GPU tensors costs one host sync per forward (one each
        if the two live on different GPUs; none for CPU tensors).
      compute: ``auto|fp32|fp16|bf16|fp8``, resolved as for ``ntxent_loss``. ``fp8`` computes in
        fp16: these kernels have no fp8 operands.
      use_mixed_precision: fp32 inputs are computed in fp16 (fp32 accumulate) if True.

    One GPU; the data-parallel form is ``parallel.sigmoid.dist_sigmoid_loss``.
    """
    h = _stack_views(h, z2)
    if _use_reference(h):
        if h.is_cuda and os.environ.get("NTXENT_ALLOW_REFERENCE", "0") != "1":
            raise RuntimeError("NTXENT_FORCE_REFERENCE requires NTXENT_ALLOW_REFERENCE=1")
        # autograd carries the gradients of tensor arguments
        t, b = (v.reshape(()).to(h.device) if isinstance(v, torch.Tensor) else v
                for v in (_one_element(temperature, "temperature"), _one_element(bias, "bias")))
        return reference.sigmoid_loss(h, t, b)
    comp = resolve_compute(h.dtype, use_mixed_precision, compute)
    if comp == "fp8":
        comp = "fp16"
    tv, bv, tau, bias_t = _scalar_args(temperature, bias)
    return SigmoidFunction.apply(h, tv, bv, comp, tau, bias_t)


class SigmoidLoss(_TemperatureModule):
    """``nn.Module`` front end: ``SigmoidLoss(temperature, bias)(z1, z2)`` or ``(h)``. One GPU.

    ``learnable_temperature=True``: as ``InfoNCELoss``, an fp32 parameter ``log_temperature``
    evaluated as ``log_temperature.exp().clamp(*temperature_bounds)`` (SigLIP's ``t`` is its
    reciprocal). ``learnable_bias=True``: the module owns an fp32 parameter ``bias``, initialised to
    ``bias``; both gradients come from the same backward.
    """

    def __init__(self, temperature: float = 0.1, bias: float = -10.0, compute: str = "auto",
                 use_mixed_precision: bool = False, learnable_temperature: bool = False,
                 temperature_bounds=(0.01, 1.0), learnable_bias: bool = False):
        super().__init__()
        self.compute = compute
        self.use_mixed_precision = use_mixed_precision
        self._init_temperature(temperature, learnable_temperature, temperature_bounds)
        self.learnable_bias = bool(learnable_bias)
        self.initial_bias = float(bias)
        if self.learnable_bias:
            self.bias = torch.nn.Parameter(torch.tensor(float(bias), dtype=torch.float32))
        else:
            self.bias = float(bias)

    def forward(self, z1: torch.Tensor, z2: Optional[torch.Tensor] = None) -> torch.Tensor:
        return sigmoid_loss(z1, self.current_temperature(), self.bias, z2=z2, compute=self.compute,
                            use_mixed_precision=self.use_mixed_precision)

    def extra_repr(self) -> str:
        return (f"temperature={self.temperature}, bias={self.initial_bias}, compute={self.compute}"
                + self._temperature_repr() + (", learnable_bias=True" if self.learnable_bias else ""))
