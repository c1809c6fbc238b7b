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

from typing import Optional

import torch

from . import _ext, reference
from .ntxent import (_reference_loss, _stack_views, _tau_grad, _tau_like, _TemperatureModule, _use_reference,
                     resolve_compute, temperature_value, temperature_wants_grad)


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
        ctx.tau = _tau_like(tau)
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
        return dh, None, None, _tau_grad(dtau, ctx.tau)


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

    One GPU; the global-batch form over a process group is ``parallel.dist_info_nce_loss``.
    """
    h = _stack_views(h, z2)
    if _use_reference(h):
        return _reference_loss(reference.info_nce_loss, h, temperature)
    comp = resolve_compute(h.dtype, use_mixed_precision, compute)
    if comp == "fp8":
        comp = "fp16"
    tau = temperature if temperature_wants_grad(temperature) else None
    return InfoNCEFunction.apply(h, temperature_value(temperature), comp, tau)


class InfoNCELoss(_TemperatureModule):
    """``nn.Module`` front end: ``InfoNCELoss(temperature)(z1, z2)`` or ``(h)``. One GPU
    (``parallel.DistInfoNCELoss`` for the data-parallel batch).

    ``learnable_temperature=True``: the module owns an fp32 parameter ``log_temperature``,
    initialised to ``log(temperature)``, and evaluates the loss at
    ``log_temperature.exp().clamp(*temperature_bounds)`` (CLIP's ``logit_scale`` is its reciprocal);
    its gradient comes from the same backward.
    """

    def __init__(self, temperature: float = 0.07, compute: str = "auto", use_mixed_precision: bool = False,
                 learnable_temperature: bool = False, temperature_bounds=(0.01, 1.0)):
        super().__init__()
        self.compute = compute
        self.use_mixed_precision = use_mixed_precision
        self._init_temperature(temperature, learnable_temperature, temperature_bounds)

    def forward(self, z1: torch.Tensor, z2: Optional[torch.Tensor] = None) -> torch.Tensor:
        return info_nce_loss(z1, self.current_temperature(), z2=z2, compute=self.compute,
                             use_mixed_precision=self.use_mixed_precision)

    def extra_repr(self) -> str:
        return f"temperature={self.temperature}, compute={self.compute}" + self._temperature_repr()
