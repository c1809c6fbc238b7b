"""Cross-view InfoNCE on MI355X: the CLIP-form two-tower loss, one GPU.

For L2-normalised towers ``A, B`` of ``N`` rows each::

    loss = (CE(A B^T / tau, arange(N)) + CE(B A^T / tau, arange(N))) / 2

i.e. NT-Xent with every same-view column masked out: a row is contrasted against the ``N`` rows of
the *other* view only (CLIP / SigLIP-style image-text training, MoCo v3). Rows are stacked as
everywhere in the package, ``h = [h1; h2]``.

Execution: prep (L2-normalise, positive logits) -> MFMA tile GEMM of the N x N block ``Z1 Z2^T``
whose epilogue reduces every tile to per-row and per-column LSE partials -> LSE merge and
deterministic loss sum; backward: prep again -> the coefficient block ``G = P12 + P21^T - 2 I`` written
once (fp32 plans in fp32; 16-bit plans as the rounded value plus the scaled residual of the rounding,
two planes of the compute dtype) -> ``G Z2`` and ``G^T Z1`` on MFMA into an fp32 slab -> grad_out/(2N
tau) scale + L2-normalisation backward (``csrc/kernels/xview_kernels.hip``).
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch

from . import _ext, reference
from .ntxent import _use_reference, resolve_compute, temperature_value, temperature_wants_grad


class InfoNCEFunction(torch.autograd.Function):
    """loss = InfoNCE(h) for stacked views h = [h1; h2] on one GPU.

    ``tau`` is None, or the one-element temperature tensor whose gradient is wanted: the backward
    then also returns dL/dtau (``xview_backward_tau``) in that tensor's dtype, shape and device."""

    @staticmethod
    def forward(ctx, h: torch.Tensor, temperature: float, compute: str, tau: Optional[torch.Tensor] = None):
        C = _ext.load()
        h = h.contiguous()
        loss, inv, lse2, cpos = C.xview_forward(h, float(temperature), compute)
        ctx.temperature = float(temperature)
        ctx.compute = compute
        ctx.tau = None if tau is None else (tau.dtype, tau.device, tau.shape)
        ctx.save_for_backward(h, inv, lse2, cpos)
        return loss

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        C = _ext.load()
        h, inv, lse2, cpos = ctx.saved_tensors
        if ctx.tau is None or not ctx.needs_input_grad[3]:
            dh = C.xview_backward(h, inv, lse2, cpos, grad_out.reshape(1), ctx.temperature, ctx.compute)
            return dh, None, None, None
        dh, dtau = C.xview_backward_tau(h, inv, lse2, cpos, grad_out.reshape(1), ctx.temperature, ctx.compute)
        dtype, device, shape = ctx.tau
        return dh, None, None, dtau.to(device=device, dtype=dtype).reshape(shape)


def info_nce_loss(h: torch.Tensor, temperature=0.07, *, z2: Optional[torch.Tensor] = None, compute: str = "auto",
                  use_mixed_precision: bool = False) -> torch.Tensor:
    """Cross-view InfoNCE of stacked views ``h = [h1; h2]`` (or ``h1=h, z2=h2``; the two may come from
    different encoders: autograd splits the gradient).

    Args:
      temperature: tau, a float or a one-element tensor. A tensor that requires grad (or has a
        ``grad_fn``, e.g. ``logit_scale.exp().reciprocal()``) receives dL/dtau from the backward, in
        its own dtype and on its own device; loss and dh are bitwise those of the same float.
      compute: ``auto|fp32|fp16|bf16|fp8``, resolved as for ``ntxent_loss``. ``fp8`` computes in
        fp16: these kernels have no fp8 operands (as the contrastive metrics).
      use_mixed_precision: fp32 inputs are computed in fp16 (fp32 accumulate) if True.

    One GPU only: there is no distributed form of this loss yet.
    """
    if z2 is not None:
        h = torch.cat([h, z2], 0)
    if h.dim() != 2 or h.shape[0] % 2:
        raise ValueError("expected stacked views [2N, d]")
    if _use_reference(h):
        if h.is_cuda and os.environ.get("NTXENT_ALLOW_REFERENCE", "0") != "1":
            raise RuntimeError("NTXENT_FORCE_REFERENCE requires NTXENT_ALLOW_REFERENCE=1")
        if isinstance(temperature, torch.Tensor):  # autograd carries the temperature's gradient
            if temperature.numel() != 1:
                raise ValueError("temperature must be a float or a one-element tensor")
            temperature = temperature.reshape(()).to(h.device)
        return reference.info_nce_loss(h, temperature)
    comp = resolve_compute(h.dtype, use_mixed_precision, compute)
    if comp == "fp8":
        comp = "fp16"
    tau = temperature if temperature_wants_grad(temperature) else None
    return InfoNCEFunction.apply(h, temperature_value(temperature), comp, tau)


class InfoNCELoss(torch.nn.Module):
    """``nn.Module`` front end: ``InfoNCELoss(temperature)(z1, z2)`` or ``(h)``. One GPU only.

    ``learnable_temperature=True``: the module owns an fp32 parameter ``log_temperature``,
    initialised to ``log(temperature)``, and evaluates the loss at
    ``log_temperature.exp().clamp(*temperature_bounds)`` (CLIP's ``logit_scale`` is its reciprocal);
    its gradient comes from the same backward.
    """

    def __init__(self, temperature: float = 0.07, compute: str = "auto", use_mixed_precision: bool = False,
                 learnable_temperature: bool = False, temperature_bounds=(0.01, 1.0)):
        super().__init__()
        self.temperature = float(temperature)
        self.compute = compute
        self.use_mixed_precision = use_mixed_precision
        self.learnable_temperature = bool(learnable_temperature)
        self.temperature_bounds = (float(temperature_bounds[0]), float(temperature_bounds[1]))
        if self.learnable_temperature:
            if not 0.0 < self.temperature_bounds[0] <= self.temperature_bounds[1]:
                raise ValueError("temperature_bounds must be 0 < low <= high")
            self.log_temperature = torch.nn.Parameter(torch.tensor(math.log(self.temperature), dtype=torch.float32))

    def current_temperature(self):
        """The temperature the next call uses: a float, or the clamped ``log_temperature.exp()``."""
        if not self.learnable_temperature:
            return self.temperature
        return self.log_temperature.exp().clamp(*self.temperature_bounds)

    def forward(self, z1: torch.Tensor, z2: Optional[torch.Tensor] = None) -> torch.Tensor:
        return info_nce_loss(z1, self.current_temperature(), z2=z2, compute=self.compute,
                             use_mixed_precision=self.use_mixed_precision)

    def metrics(self, z1: torch.Tensor, z2: Optional[torch.Tensor] = None, topk=(1, 5)):
        """Contrastive metrics of the same inputs (``ops.metrics.contrastive_metrics``); they rank the
        positive against all ``2N - 2`` other rows, same-view rows included."""
        from .metrics import contrastive_metrics

        return contrastive_metrics(z1, z2=z2, topk=topk, compute=self.compute,
                                   use_mixed_precision=self.use_mixed_precision)

    def extra_repr(self) -> str:
        s = f"temperature={self.temperature}, compute={self.compute}"
        if self.learnable_temperature:
            s += f", learnable_temperature=True, temperature_bounds={self.temperature_bounds}"
        return s
