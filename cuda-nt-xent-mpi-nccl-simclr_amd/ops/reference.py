"""Pure-PyTorch NT-Xent oracle (CPU or GPU, any dtype; fp64 for gradchecks).

This is the *correct* SimCLR NT-Xent that the reference intends. The
reference itself computes something else (self-similarity diagonal of a scrambled GEMM,
``src/ntxent_kernel.cu:117,161-173``) and its backward ignores ``grad_out``
(``src/ntxent_kernel.cu:221``), so parity targets these formulas, not its outputs.

Notation: ``h = [h1; h2]`` of shape ``[2N, d]``; ``z = h / max(||h||, eps)``;
``S = z z^T / tau`` with the diagonal masked; positive ``p(i) = (i + N) mod 2N``;
``lse_i = log sum_{j != i} exp S_ij``; ``loss = mean_i (lse_i - S_{i,p(i)})``.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

EPS = 1e-12


def normalize(h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Return (z, inv_norm) with z = h * inv_norm, inv_norm = 1/max(||h||, eps)."""
    inv = 1.0 / h.norm(dim=1).clamp_min(EPS)
    return h * inv.unsqueeze(1), inv


def positive_index(rows: int, device=None) -> torch.Tensor:
    n = rows // 2
    return (torch.arange(rows, device=device) + n) % rows


def logits(h: torch.Tensor, temperature: float) -> torch.Tensor:
    z, _ = normalize(h)
    S = z @ z.t() / temperature
    mask = torch.eye(h.shape[0], dtype=torch.bool, device=h.device)
    return S.masked_fill(mask, float("-inf"))


def ntxent_loss(h: torch.Tensor, temperature: float = 0.07) -> torch.Tensor:
    """Autograd-capable NT-Xent on stacked views ``h = [h1; h2]``."""
    if h.dim() != 2 or h.shape[0] % 2:
        raise ValueError("h must be [2N, d] with stacked views")
    S = logits(h, temperature)
    pos = positive_index(h.shape[0], h.device)
    return torch.nn.functional.cross_entropy(S, pos, reduction="mean")


def ntxent_loss_pair(z1: torch.Tensor, z2: torch.Tensor, temperature: float = 0.07) -> torch.Tensor:
    return ntxent_loss(torch.cat([z1, z2], 0), temperature)


def ntxent_stats(h: torch.Tensor, temperature: float = 0.07):
    """(loss, lse[2N], pos_logit[2N]) in the dtype of h."""
    S = logits(h, temperature)
    lse = torch.logsumexp(S, dim=1)
    pos = positive_index(h.shape[0], h.device)
    pl = S.gather(1, pos.unsqueeze(1)).squeeze(1)
    return (lse - pl).mean(), lse, pl


def ntxent_backward_analytic(h: torch.Tensor, temperature: float, grad_out: float | torch.Tensor = 1.0,
                             lse: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Closed-form gradient via the symmetric trick (what the HIP backward implements).

    C = P + P^T - 2 I_pos, dL/dz = C z / (2N tau), dL/dh = inv (dz - z (z . dz)).
    """
    R = h.shape[0]
    z, inv = normalize(h)
    S = logits(h, temperature)
    if lse is None:
        lse = torch.logsumexp(S, dim=1)
    P = torch.exp(S - lse.unsqueeze(1))
    pos = positive_index(R, h.device)
    C = P + P.t()
    C[torch.arange(R, device=h.device), pos] -= 2.0
    dz = (C @ z) * (torch.as_tensor(grad_out, dtype=h.dtype, device=h.device) / (R * temperature))
    dot = (z * dz).sum(1, keepdim=True)
    return inv.unsqueeze(1) * (dz - z * dot)


def ntxent_temperature_grad_analytic(h: torch.Tensor, temperature: float,
                                     grad_out: float | torch.Tensor = 1.0) -> torch.Tensor:
    """Closed-form d loss / d tau (what the HIP ``tau_grad`` launch implements), a 0-d tensor.

    With R = 2N rows, cos = z z^T and C = P + P^T - 2 I_pos:
    dL/dtau = -(1 / (2 R tau^2)) sum_i dot_i, dot_i = sum_j C_ij cos_ij = z_i . (C z)_i,
    the per-row scalar of the normalisation backward.
    """
    R = h.shape[0]
    tau = float(temperature)
    z, _ = normalize(h)
    S = logits(h, tau)
    P = torch.exp(S - torch.logsumexp(S, dim=1, keepdim=True))
    pos = positive_index(R, h.device)
    C = P + P.t()
    C[torch.arange(R, device=h.device), pos] -= 2.0
    dot = (z * (C @ z)).sum(1)
    return -torch.as_tensor(grad_out, dtype=h.dtype, device=h.device) * dot.sum() / (2.0 * R * tau * tau)


# ---------------------------------------------------------------------------------------
# Cross-view InfoNCE (the CLIP form): a row's columns are the rows of the other view only.
# ---------------------------------------------------------------------------------------
def cross_view_logits(h: torch.Tensor, temperature) -> torch.Tensor:
    """``z z^T / tau`` with every same-view entry (the diagonal included) masked to -inf."""
    R = h.shape[0]
    z, _ = normalize(h)
    view = torch.arange(R, device=h.device) >= R // 2
    return (z @ z.t() / temperature).masked_fill(view.unsqueeze(0) == view.unsqueeze(1), float("-inf"))


def info_nce_loss(h: torch.Tensor, temperature=0.07) -> torch.Tensor:
    """Autograd-capable cross-view InfoNCE on stacked views ``h = [h1; h2]``: NT-Xent with the
    same-view columns masked, which is ``(CE(A B^T / tau) + CE(B A^T / tau)) / 2`` of the unit towers."""
    if h.dim() != 2 or h.shape[0] % 2:
        raise ValueError("h must be [2N, d] with stacked views")
    S = cross_view_logits(h, temperature)
    return torch.nn.functional.cross_entropy(S, positive_index(h.shape[0], h.device), reduction="mean")


def _info_nce_coefficients(h: torch.Tensor, tau: float):
    """(z, inv, C) with C = M o (P + P^T) - 2 I_pos, M the cross-view mask (P is zero off it)."""
    R = h.shape[0]
    z, inv = normalize(h)
    S = cross_view_logits(h, tau)
    P = torch.exp(S - torch.logsumexp(S, dim=1, keepdim=True))
    C = P + P.t()
    C[torch.arange(R, device=h.device), positive_index(R, h.device)] -= 2.0
    return z, inv, C


def info_nce_backward_analytic(h: torch.Tensor, temperature: float,
                               grad_out: float | torch.Tensor = 1.0) -> torch.Tensor:
    """Closed-form gradient of ``info_nce_loss`` (what the HIP backward implements):
    dL/dz = C z / (R tau), dL/dh = inv (dz - z (z . dz))."""
    R = h.shape[0]
    z, inv, C = _info_nce_coefficients(h, float(temperature))
    dz = (C @ z) * (torch.as_tensor(grad_out, dtype=h.dtype, device=h.device) / (R * float(temperature)))
    dot = (z * dz).sum(1, keepdim=True)
    return inv.unsqueeze(1) * (dz - z * dot)


def info_nce_temperature_grad_analytic(h: torch.Tensor, temperature: float,
                                       grad_out: float | torch.Tensor = 1.0) -> torch.Tensor:
    """Closed-form d loss / d tau of ``info_nce_loss``, a 0-d tensor:
    -(1 / (2 R tau^2)) sum_i dot_i with dot_i = sum_j C_ij cos_ij = z_i . (C z)_i."""
    R = h.shape[0]
    tau = float(temperature)
    z, _, C = _info_nce_coefficients(h, tau)
    dot = (z * (C @ z)).sum(1)
    return -torch.as_tensor(grad_out, dtype=h.dtype, device=h.device) * dot.sum() / (2.0 * R * tau * tau)


# ---------------------------------------------------------------------------------------
# Contrastive metrics: the rank of each row's positive among its negatives.
# ---------------------------------------------------------------------------------------
def _negatives_mask(rows: int, device=None) -> torch.Tensor:
    """[R, R] bool: True where column j is a negative of row i (j != i and j != p(i))."""
    idx = torch.arange(rows, device=device)
    keep = torch.ones(rows, rows, dtype=torch.bool, device=device)
    keep[idx, idx] = False
    keep[idx, positive_index(rows, device)] = False
    return keep


def _rank_parts(z_unit: torch.Tensor, delta: float):
    """(lo, hi, t, hard) of unit rows: negatives with cos > t + delta / cos > t - delta, the positive
    cosine t and the largest negative cosine (-inf without negatives)."""
    if z_unit.dim() != 2 or z_unit.shape[0] % 2:
        raise ValueError("expected stacked views [2N, d]")
    R = z_unit.shape[0]
    cos = z_unit @ z_unit.t()
    t = cos.gather(1, positive_index(R, z_unit.device).unsqueeze(1))
    keep = _negatives_mask(R, z_unit.device)
    lo = ((cos > t + delta) & keep).sum(1)
    hi = ((cos > t - delta) & keep).sum(1)
    hard = cos.masked_fill(~keep, float("-inf")).max(1).values
    return lo, hi, t.squeeze(1), hard


def positive_rank_bounds(z_unit: torch.Tensor, delta: float):
    """(lo, hi) for unit rows ``z_unit`` ([2N, d], used as they are): ``lo`` counts the negatives
    with ``cos > t + delta`` and ``hi`` those with ``cos > t - delta``, t being the positive cosine.
    An implementation whose cosines are all within ``delta / 2`` of these has ``lo <= rank <= hi``."""
    lo, hi, _, _ = _rank_parts(z_unit, delta)
    return lo, hi


def positive_rank(h: torch.Tensor):
    """(rank int32 [2N], pos_cos [2N], hard_neg_cos [2N]) of stacked views ``h = [h1; h2]``, in the
    dtype of ``h``: rank_i = #{ j : j != i, j != p(i), cos_ij > cos_i,p(i) } (strict), so 0 means
    the positive is the most similar row. hard_neg_cos is -inf when there are no negatives."""
    if h.dim() != 2 or h.shape[0] % 2:
        raise ValueError("expected stacked views [2N, d]")
    z, _ = normalize(h)
    lo, _, t, hard = _rank_parts(z, 0.0)
    return lo.to(torch.int32), t, hard


# ---------------------------------------------------------------------------------------
# Data-parallel layout: rank r holds h_r = [h1_r; h2_r] (2n rows); positives are rank-local.
# ---------------------------------------------------------------------------------------
def global_pair_order(shards: Sequence[torch.Tensor]) -> torch.Tensor:
    """Re-stack per-rank shards into the single-process [view1; view2] layout (same pairs)."""
    n = shards[0].shape[0] // 2
    v1 = torch.cat([s[:n] for s in shards], 0)
    v2 = torch.cat([s[n:] for s in shards], 0)
    return torch.cat([v1, v2], 0)


def sharded_forward_backward(shards: Sequence[torch.Tensor], temperature: float,
                             grad_out: float = 1.0) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """Simulate the W-rank algorithm in one process: each rank uses only its rows, the
    gathered normalised embeddings and the gathered LSE (no column-gradient exchange)."""
    W = len(shards)
    R = shards[0].shape[0]
    n = R // 2
    zs, invs = zip(*[normalize(s) for s in shards])
    z_all = torch.cat(zs, 0)
    N2 = W * R
    lses, losses = [], []
    for r in range(W):
        S = zs[r] @ z_all.t() / temperature
        own = torch.arange(R, device=S.device) + r * R
        S[torch.arange(R), own] = float("-inf")
        lse = torch.logsumexp(S, 1)
        pos = (torch.arange(R) + n) % R + r * R
        losses.append((lse - S[torch.arange(R), pos]).sum())
        lses.append(lse)
    lse_all = torch.cat(lses)
    loss = torch.stack(losses).sum() / N2
    grads = []
    for r in range(W):
        S = zs[r] @ z_all.t() / temperature
        own = torch.arange(R) + r * R
        Pr = torch.exp(S - lses[r].unsqueeze(1))
        Pc = torch.exp(S - lse_all.unsqueeze(0))
        C = Pr + Pc
        C[torch.arange(R), own] = 0.0
        pos = (torch.arange(R) + n) % R + r * R
        C[torch.arange(R), pos] -= 2.0
        dz = C @ z_all * (grad_out / (N2 * temperature))
        z = zs[r]
        dot = (z * dz).sum(1, keepdim=True)
        grads.append(invs[r].unsqueeze(1) * (dz - z * dot))
    return loss, grads


# ---------------------------------------------------------------------------------------
# What the reference computes as written (for documentation / contrast tests only).
# ---------------------------------------------------------------------------------------
def reference_as_written_forward(z: torch.Tensor, T: float) -> torch.Tensor:
    """Emulates src/ntxent_kernel.cu:160-200 (column-major cuBLAS with lda=2B on row-major
    data, self-diagonal target). Kept to document why parity targets the correct math."""
    B, D = z.shape
    zc = torch.cat([z, z], 0)  # :161
    A = zc.reshape(-1)[: 2 * B * D].reshape(D, 2 * B).t()  # lda=2B read of row-major memory
    L = A @ A.t() / T
    P = torch.softmax(L, dim=1)
    return -torch.log(torch.diagonal(P)).mean()


def flops_fwd_bwd(rows_local: int, rows_global: int, dim: int, symmetric_local: bool = True,
                  symmetric_global: bool = False) -> float:
    """MFMA FLOPs of one rank's fwd+bwd (store mode): fwd S GEMM (upper-triangular in the
    own-rank block; with ``symmetric_global`` each cross-rank block counted once per pair, i.e.
    half per rank, as parallel/symmetric.py executes it) + dZ GEMM. For TFLOP/s reporting."""
    own = rows_local * rows_local * dim * 2.0
    remote = rows_local * (rows_global - rows_local) * dim * 2.0
    fwd = (own / 2 if symmetric_local else own) + (remote / 2 if symmetric_global else remote)
    bwd = rows_local * rows_global * dim * 2.0
    return fwd + bwd


def expected_random_loss(rows: int) -> float:
    """Loss of an uninformative model: log(2N - 1)."""
    return math.log(rows - 1)
