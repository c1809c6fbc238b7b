"""NT-Xent loss on MI355X: autograd Function, functional API and ``nn.Module``.

The reference exposes raw ``forward``/``backward`` ops with no autograd link
(``src/binding_new.cpp:4-21``); its tests nevertheless call ``loss.backward()``
(``tests/test_forward.cpp:29-38``). Here the HIP kernels are wrapped in a
``torch.autograd.Function`` so that works, and the backward honours ``grad_out``.

Execution (single process; see ``parallel.distributed`` for global-batch negatives):
  forward : prep (L2-normalise, quantise to the compute dtype, positive logits)
            -> fused MFMA similarity GEMM with per-tile online LSE partials (upper-triangular
               tiles only, S is symmetric) -> LSE merge + deterministic loss reduction
  backward: coefficient pass C = P + P^T - 2 I_pos (in place over the kept cosines, or
            recomputed by the GEMM when ``keep_logits=False``) -> MFMA dZ = C Z
            -> fused grad_out/(2N tau) scale + L2-normalisation backward.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch

from . import _ext, reference

_VALID_COMPUTE = ("auto", "fp32", "fp16", "bf16", "fp8")


def _use_reference(h: torch.Tensor) -> bool:
    if not h.is_cuda:
        return True
    return os.environ.get("NTXENT_FORCE_REFERENCE", "0") == "1"


def resolve_compute(dtype: torch.dtype, use_mixed_precision: bool = False, compute: str = "auto") -> str:
    """Compute-dtype policy (mirrors the C++ one): fp32 inputs stay exact fp32 unless
    mixed precision is requested; reduced precision is fp16 (normalised rows in [-1, 1])."""
    if compute not in _VALID_COMPUTE:
        raise ValueError(f"compute must be one of {_VALID_COMPUTE}")
    if compute != "auto":
        return compute
    if dtype == torch.float32 and not use_mixed_precision:
        return "fp32"
    return "fp16"


def temperature_value(temperature) -> float:
    """tau as a host float. A one-element tensor is read with ``.item()``: one host sync when it
    lives on the GPU, none for a CPU tensor."""
    if isinstance(temperature, torch.Tensor):
        if temperature.numel() != 1:
            raise ValueError("temperature must be a float or a one-element tensor")
        return float(temperature.detach().item())
    return float(temperature)


def temperature_wants_grad(temperature) -> bool:
    """True for a tensor temperature autograd tracks: a leaf that requires grad, or a result with
    a ``grad_fn`` such as ``log_scale.exp()``."""
    return isinstance(temperature, torch.Tensor) and (temperature.requires_grad or temperature.grad_fn is not None)


def refuse_temperature_grad(temperature, where: str) -> None:
    """The data-parallel paths do not all-reduce the per-rank dL/dtau partials yet: refuse a
    temperature that requires grad instead of detaching it silently."""
    if temperature_wants_grad(temperature):
        raise NotImplementedError(
            f"{where}: a temperature that requires grad is supported on one GPU only (ntxent_loss); the "
            "distributed paths do not reduce its gradient across ranks. Pass a float or a detached tensor.")


# ---- what ntxent_loss and ops.infonce.info_nce_loss share ---------------------------------
def _stack_views(h: torch.Tensor, z2: Optional[torch.Tensor]) -> torch.Tensor:
    """``[h; z2]`` (or ``h`` as it is), checked to be stacked views ``[2N, d]``."""
    if z2 is not None:
        h = torch.cat([h, z2], 0)
    if h.dim() != 2 or h.shape[0] % 2:
        raise ValueError("expected stacked views [2N, d]")
    return h


def _reference_loss(oracle, h: torch.Tensor, temperature) -> torch.Tensor:
    """The eager ``oracle(h, temperature)`` of ``ops.reference`` for rows ``_use_reference`` sends there."""
    if h.is_cuda and os.environ.get("NTXENT_ALLOW_REFERENCE", "0") != "1":
        raise RuntimeError("NTXENT_FORCE_REFERENCE requires NTXENT_ALLOW_REFERENCE=1")
    if isinstance(temperature, torch.Tensor):  # autograd carries the temperature's gradient
        if temperature.numel() != 1:
            raise ValueError("temperature must be a float or a one-element tensor")
        temperature = temperature.reshape(()).to(h.device)
    return oracle(h, temperature)


def _tau_like(tau: Optional[torch.Tensor]):
    """What an autograd Function keeps of the temperature tensor whose gradient is wanted."""
    return None if tau is None else (tau.dtype, tau.device, tau.shape)


def _tau_grad(dtau: torch.Tensor, like) -> torch.Tensor:
    """The kernels' 0-d fp32 dL/dtau in the temperature's own dtype, device and shape (``_tau_like``)."""
    dtype, device, shape = like
    return dtau.to(device=device, dtype=dtype).reshape(shape)


class _TemperatureModule(torch.nn.Module):
    """What NTXentLoss and InfoNCELoss share: the fixed or learnable temperature and ``metrics``."""

    def _init_temperature(self, temperature, learnable_temperature, temperature_bounds) -> None:
        self.temperature = float(temperature)
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

    def metrics(self, z1: torch.Tensor, z2: Optional[torch.Tensor] = None, topk=(1, 5)):
        """Contrastive metrics of the same inputs ``forward`` takes (``ops.metrics.contrastive_metrics``:
        ``top{k}``, ``mean_rank``, ``pos_cos``, ``hard_neg_cos``, ``negatives``) with the module's
        ``compute`` and ``use_mixed_precision``; no gradient, and independent of the temperature.
        The positive is ranked against all ``2N - 2`` other rows, same-view rows included; in a
        distributed module against this rank's own ``2n - 2`` only, not against the global batch."""
        from .metrics import contrastive_metrics

        return contrastive_metrics(z1, z2=z2, topk=topk, compute=self.compute,
                                   use_mixed_precision=self.use_mixed_precision)

    def _temperature_repr(self) -> str:
        if not self.learnable_temperature:
            return ""
        return f", learnable_temperature=True, temperature_bounds={self.temperature_bounds}"


class NTXentFunction(torch.autograd.Function):
    """loss = NTXent(h) for stacked views h = [h1; h2] on one GPU.

    ``tau`` is None, or the one-element temperature tensor whose gradient is wanted: the backward
    then also returns dL/dtau (``fused_backward_tau``) in that tensor's dtype, shape and device."""

    @staticmethod
    def forward(ctx, h: torch.Tensor, temperature: float, compute: str, keep_logits: bool,
                tau: Optional[torch.Tensor] = None):
        C = _ext.load()
        h = h.contiguous()
        loss, zq, zqt, inv, lse2, sc, cpos = C.fused_forward(h, float(temperature), compute, bool(keep_logits))
        ctx.temperature = float(temperature)
        ctx.tau = _tau_like(tau)
        ctx.sc = sc if keep_logits else None  # released by the first backward
        ctx.save_for_backward(h, zq, zqt, inv, lse2, cpos)
        ctx.mark_non_differentiable()
        return loss

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        C = _ext.load()
        h, zq, zqt, inv, lse2, cpos = ctx.saved_tensors
        sc, ctx.sc = ctx.sc, None  # a second backward (retain_graph) recomputes the cosines
        if ctx.tau is None or not ctx.needs_input_grad[4]:
            dh = C.fused_backward(h, zq, zqt, inv, lse2, sc, cpos, grad_out.reshape(1), ctx.temperature)
            return dh, None, None, None, None
        dh, dtau = C.fused_backward_tau(h, zq, zqt, inv, lse2, sc, cpos, grad_out.reshape(1), ctx.temperature)
        return dh, None, None, None, _tau_grad(dtau, ctx.tau)


def ntxent_loss(h: torch.Tensor, temperature=0.07, *, use_mixed_precision: bool = False,
                compute: str = "auto", keep_logits: bool = True, z2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """NT-Xent loss of stacked views ``h = [h1; h2]`` (or ``h1=h, z2=h2``).

    Args:
      temperature: tau, a float or a one-element tensor. A tensor that requires grad (or has a
        ``grad_fn``, e.g. ``log_scale.exp()``) receives dL/dtau from the backward, in its own dtype
        and on its own device; loss, dh and the plan are bitwise those of the same float. The
        kernels take tau by value, so reading a GPU tensor's value costs one host sync per forward;
        a CPU tensor costs none.
      use_mixed_precision: fp32 inputs are computed in fp16 (fp32 accumulate) if True.
      compute: override the compute dtype: ``auto|fp32|fp16|bf16|fp8``. ``fp8`` runs the forward
        similarity GEMM on block-scaled e4m3 MFMA (per-row amax power-of-two scales) and the backward in fp16; the
        loss is that of the fp8-quantised rows (logit error ~1e-2 at tau=0.07, see
        tests/test_gpu_fp8.py).
      keep_logits: keep the cosine tiles (compute dtype) between forward and backward
        (default; saves one similarity GEMM). False recomputes them in the backward.
    """
    h = _stack_views(h, z2)
    if _use_reference(h):
        return _reference_loss(reference.ntxent_loss, h, temperature)
    comp = resolve_compute(h.dtype, use_mixed_precision, compute)
    keep = bool(keep_logits) or comp == "fp8"
    if temperature_wants_grad(temperature):
        return NTXentFunction.apply(h, temperature_value(temperature), comp, keep, temperature)
    return NTXentFunction.apply(h, temperature_value(temperature), comp, keep, None)


class NTXentLoss(_TemperatureModule):
    """``nn.Module`` front end: ``NTXentLoss(temperature)(z1, z2)`` or ``(h)``.

    With ``distributed=True`` negatives come from the whole data-parallel group over RCCL/xGMI
    (``negatives``: "allgather", "symmetric" or "ring"), see :mod:`parallel`.

    ``learnable_temperature=True`` (one GPU only): the module owns an fp32 parameter
    ``log_temperature``, initialised to ``log(temperature)``, and evaluates the loss at
    ``log_temperature.exp().clamp(*temperature_bounds)``; its gradient comes from the same backward.
    """

    def __init__(self, temperature: float = 0.07, use_mixed_precision: bool = False, compute: str = "auto",
                 keep_logits: bool = True, distributed: bool = False, group=None, negatives: str = "allgather",
                 learnable_temperature: bool = False, temperature_bounds=(0.01, 1.0)):
        super().__init__()
        self.negatives = negatives
        self.use_mixed_precision = use_mixed_precision
        self.compute = compute
        self.keep_logits = keep_logits
        self.distributed = distributed
        self.group = group
        if learnable_temperature and distributed:
            raise NotImplementedError(
                "NTXentLoss: learnable_temperature is supported on one GPU only; the distributed paths do "
                "not reduce the temperature gradient across ranks")
        self._init_temperature(temperature, learnable_temperature, temperature_bounds)

    def forward(self, z1: torch.Tensor, z2: Optional[torch.Tensor] = None) -> torch.Tensor:
        h = z1 if z2 is None else torch.cat([z1, z2], 0)
        if self.distributed:
            from ..parallel.distributed import dist_ntxent_loss

            return dist_ntxent_loss(h, self.temperature, group=self.group, compute=self.compute,
                                    use_mixed_precision=self.use_mixed_precision, keep_logits=self.keep_logits,
                                    negatives=self.negatives)
        return ntxent_loss(h, self.current_temperature(), use_mixed_precision=self.use_mixed_precision,
                           compute=self.compute, keep_logits=self.keep_logits)

    def extra_repr(self) -> str:
        return (f"temperature={self.temperature}, compute={self.compute}, distributed={self.distributed}"
                + self._temperature_repr())


# ---- reference-compatible raw op API (src/binding_new.cpp:5-20) --------------------------
def forward(z: torch.Tensor, T: float, use_mixed_precision: bool = False) -> torch.Tensor:
    return _ext.load().forward(z, float(T), use_mixed_precision)


def forward_with_stats(z: torch.Tensor, T: float, use_mixed_precision: bool = False):
    return tuple(_ext.load().forward_with_stats(z, float(T), use_mixed_precision))


def backward(z: torch.Tensor, softmax: torch.Tensor, grad_out: torch.Tensor, T: float,
             use_mixed_precision: bool = False, want_grad_logits: bool = False):
    """(grad_z, grad_logits). `softmax` may be the LSE that forward_with_stats returned for this
    very z (then the row statistics are not recomputed); grad_logits = dL/dS is built only when
    want_grad_logits is set (else an empty tensor)."""
    return tuple(_ext.load().backward(z, softmax, grad_out, float(T), use_mixed_precision, want_grad_logits))


def check_tensor_core_support() -> bool:
    try:
        return bool(_ext.load(build_if_missing=False).check_tensor_core_support())
    except Exception:
        return False


check_matrix_core_support = check_tensor_core_support
