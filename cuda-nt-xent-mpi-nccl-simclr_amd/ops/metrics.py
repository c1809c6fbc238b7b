"""Contrastive metrics on MI355X: the rank of every row's positive among its negatives.

NT-Xent loss is hard to read while training: its floor moves with the batch size and the
temperature. What shows whether each row's positive is winning is contrastive accuracy: top-1 is
how often the positive is the most similar row, top-5 how often it is among the five most similar.
Both follow from ``rank_i = #{ j : j != i, j != p(i), cos_ij > cos_i,p(i) }`` (strict), which does
not depend on the temperature and is an integer, so it is bitwise repeatable.

On the GPU the rank comes from a kernel of its own (``csrc/kernels/rank_kernels.hip``): the row
prologue, then a similarity GEMM over the upper-triangular tiles whose epilogue compares and
counts; no 2N x 2N data is stored. The launch is opt-in: nothing in the loss, its backward or
the timed training step calls it, and it reads none of their buffers.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _ext, reference
from .ntxent import _use_reference, resolve_compute


def _stack(h: torch.Tensor, z2: Optional[torch.Tensor]) -> torch.Tensor:
    if z2 is not None:
        h = torch.cat([h, z2], 0)
    if h.dim() != 2 or h.shape[0] % 2 or h.shape[0] == 0:
        raise ValueError("expected stacked views [2N, d]")
    return h.detach()


def positive_rank(h: torch.Tensor, *, z2: Optional[torch.Tensor] = None, compute: str = "auto",
                  use_mixed_precision: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(rank, pos_cos, hard_neg_cos)`` of stacked views ``h = [h1; h2]`` (or ``h1=h, z2=h2``).

    With ``p(i) = (i + N) mod 2N`` and cosines of the L2-normalised rows:
      rank[i]         int32: negatives ``j`` (``j != i``, ``j != p(i)``) with ``cos_ij > cos_i,p(i)``,
                      strictly; 0 means the positive is the most similar row
      pos_cos[i]      fp32: ``cos_i,p(i)``
      hard_neg_cos[i] fp32: the largest negative cosine (``-inf`` when ``2N == 2``)

    Runs under ``torch.no_grad()`` on ``h.detach()``. ``compute`` resolves as for ``ntxent_loss``
    (fp32 inputs stay exact fp32; ``"fp8"`` computes in fp16: the rank kernel has no fp8 operands).
    Ties and near-ties follow the compute dtype's rounding of the unit rows. CPU tensors (and
    ``NTXENT_FORCE_REFERENCE=1`` with ``NTXENT_ALLOW_REFERENCE=1``) use the PyTorch oracle in the
    dtype of ``h``.
    """
    with torch.no_grad():
        h = _stack(h, z2)
        comp = resolve_compute(h.dtype, use_mixed_precision, compute)
        if _use_reference(h):
            if h.is_cuda and os.environ.get("NTXENT_ALLOW_REFERENCE", "0") != "1":
                raise RuntimeError("NTXENT_FORCE_REFERENCE requires NTXENT_ALLOW_REFERENCE=1")
            rank, pos, hard = reference.positive_rank(h)
            return rank, pos.float(), hard.float()
        rank, pos, hard = _ext.load().positive_rank(h.contiguous(), comp, False)
        return rank, pos, hard


def contrastive_metrics(h: torch.Tensor, *, z2: Optional[torch.Tensor] = None, topk: Sequence[int] = (1, 5),
                        compute: str = "auto", use_mixed_precision: bool = False) -> Dict[str, torch.Tensor]:
    """Contrastive accuracy and friends of stacked views, as 0-d tensors on the device of ``h``:

      ``top{k}``       fraction of rows whose positive is among the k most similar (``rank < k``)
      ``mean_rank``    mean of ``rank``
      ``pos_cos``      mean positive cosine
      ``hard_neg_cos`` mean over the rows of the largest negative cosine
      ``negatives``    ``2N - 2``, the negatives each row is ranked against (int64)

    ``top{k}`` and ``mean_rank`` are derived from :func:`positive_rank`'s integer ``rank`` (no host
    sync here). Arguments as for :func:`positive_rank`.
    """
    ks = [int(k) for k in topk]
    if any(k < 1 for k in ks):
        raise ValueError("topk entries must be >= 1")
    rank, pos, hard = positive_rank(h, z2=z2, compute=compute, use_mixed_precision=use_mixed_precision)
    with torch.no_grad():
        out = {f"top{k}": (rank < k).float().mean() for k in ks}
        out["mean_rank"] = rank.float().mean()
        out["pos_cos"] = pos.mean()
        out["hard_neg_cos"] = hard.mean()
        out["negatives"] = torch.full((), rank.numel() - 2, dtype=torch.int64, device=rank.device)
    return out
