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
# Pairwise sigmoid loss (the SigLIP form): every one of the N x N pairs is a binary term.
# ---------------------------------------------------------------------------------------
def _sigmoid_pairs(h: torch.Tensor, temperature, bias):
    """(A, B, inv, x) of stacked views: the unit towers and ``x_ij = a_i . b_j / tau + bias``."""
    if h.dim() != 2 or h.shape[0] % 2:
        raise ValueError("h must be [2N, d] with stacked views")
    n = h.shape[0] // 2
    z, inv = normalize(h)
    return z[:n], z[n:], inv, z[:n] @ z[n:].t() / temperature + bias


def sigmoid_loss(h: torch.Tensor, temperature=0.1, bias=-10.0) -> torch.Tensor:
    """Autograd-capable pairwise sigmoid loss on stacked views ``h = [h1; h2]``:
    ``(1 / N) sum_ij softplus(-s_ij x_ij)`` with ``s_ii = +1`` and ``s_ij = -1`` otherwise (SigLIP's
    loss with ``t = 1 / tau``). ``temperature`` and ``bias`` may be floats or 0-d tensors."""
    n = h.shape[0] // 2
    _, _, _, x = _sigmoid_pairs(h, temperature, bias)
    s = 2.0 * torch.eye(n, dtype=h.dtype, device=h.device) - 1.0
    return torch.nn.functional.softplus(-s * x).sum() / n


def sigmoid_backward_analytic(h: torch.Tensor, temperature: float, bias: float,
                              grad_out: float | torch.Tensor = 1.0):
    """Closed-form ``(dh, dtau, dbias)`` of ``sigmoid_loss`` (what the HIP backward implements). With
    ``G_ij = sigmoid(x_ij)`` off the diagonal and ``G_ii = -sigmoid(-x_ii)`` (formed directly, not as
    ``sigmoid - 1``): dL/dA = G B / (N tau), dL/dB = G^T A / (N tau), dL/dbias = sum G / N,
    dL/dtau = -sum G o cos / (N tau^2); dL/dh = inv (dz - z (z . dz))."""
    n = h.shape[0] // 2
    tau = float(temperature)
    a, b, inv, x = _sigmoid_pairs(h, tau, float(bias))
    eye = torch.eye(n, dtype=torch.bool, device=h.device)
    G = torch.where(eye, -torch.sigmoid(-x), torch.sigmoid(x))
    go = torch.as_tensor(grad_out, dtype=h.dtype, device=h.device)
    z = torch.cat([a, b], 0)
    dz = torch.cat([G @ b, G.t() @ a], 0) * (go / (n * tau))
    dot = (z * dz).sum(1, keepdim=True)
    dh = inv.unsqueeze(1) * (dz - z * dot)
    dtau = -go * (G * (a @ b.t())).sum() / (n * tau * tau)
    return dh, dtau, go * G.sum() / n


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
# Planted-pair probes: inputs on which ONE element (i, j) of the 2N x 2N square carries a large
# share of two rows' gradients, so a test can see an error in that one element.
# ---------------------------------------------------------------------------------------
def stacked_to_pair_order(blocks: int, rows_per_block: int) -> torch.Tensor:
    """Index map from the rank-stacked layout (``blocks`` shards ``[h1_r; h2_r]`` of
    ``rows_per_block`` rows, one after the other) to ``global_pair_order``: row k of the stacked
    rows is row ``map[k]`` of the re-stacked ``[view1; view2]``."""
    n = rows_per_block // 2
    k = torch.arange(blocks * rows_per_block)
    r, l = k // rows_per_block, k % rows_per_block
    return torch.where(l < n, r * n + l, blocks * n + r * n + (l - n))


def boundary_probes(rows: int, tile: int, *, blocks: int = 1, cross_view: bool = False,
                    return_labels: bool = False):
    """Probes ``(i, j)``, j a negative of i, at the elements where a tiled kernel's index arithmetic
    can be off by one. ``tile`` is the kernel's tile edge. ``rows`` is the row count of one block
    ``[view1; view2]``; with ``blocks = W`` the rows are W such blocks stacked (the layout the
    data-parallel kernels index: each rank's rows padded to whole tiles, positives rank-local), the
    indices count through the stacked rows (``stacked_to_pair_order`` maps them), every block gets
    the whole list and pairs across blocks are added. ``cross_view``: only pairs of rows of
    different views (cross-view InfoNCE masks the others), in both directions.

    Rules (asserted by tests/test_probes_cpu.py): every row occurs in at most one probe, no probe's
    i is another's j, and no probe row is the positive of another probe row. A candidate that
    breaks one is skipped and the next candidate of its category is tried.

    Categories (labels, with ``return_labels`` a tuple of them per probe):

    * ``self-up`` / ``self-lo``: ``(m-1, m)`` and ``(m+2, m+1)`` beside the self mask, m a multiple of
      16 (``@16``), 64 (``@64``), the tile (``@tile``), and the first row of the last tile (``@last``).
      Cross-view: the same elements of the N x N block, ``(m-1, p(m))`` and ``(p(m+2), m+1)``, which
      there lie beside the positive.
    * ``pos+1`` / ``pos-1``: ``(a, p(a)+1)`` and ``(a', p(a')-1)`` with a, a' in three different tiles.
    * ``seam``: ``(n-1, n)`` and ``(n+2, n-2)``.
    * ``last-row`` ``(R-1, x)``, ``last-col`` ``(x, R-2)``, ``first-row`` ``(0, y)``.
    * ``corner-up``: the first rows of tile I with the last columns of tile J > I, and the last rows of
      I with the first columns of J, each inside the corner's 16 x 16 fragment (the corner elements
      themselves belong to the edge probes); ``corner-lo``: the same two corners of the mirror tile
      (J, I). I is the first tile and J the last.
    * ``cross-block`` (blocks > 1), for each block a and the next one b: two pairs (i in a, j in b)
      near the first-row / last-column and last-row / first-column corners of a's first tile row
      (``upper``), two pairs (i in b, j in a) near the mirrored corners (``mirror``), and one of the
      last rows of a with a row of b (``boundary``). Cross-view (the distributed InfoNCE kernels: a
      row's columns are the other view's rows of EVERY block, the positive only in its own), in each
      direction (i in a, j in b) and (i in b, j in a), the sides alternating: j at the local index of
      i's positive, the other block's would-be positive that must count as a plain negative
      (``would-be``), its neighbours (``pos+1`` / ``pos-1``), the last valid local column of a block,
      n-1 or the nearest one the rules leave free (``last-col``), and the first, 0 or the nearest free
      one (``first-col``).

    Row R-1 is the positive of row n-1, row 0 of row n and row R-2 of row n-2, so the third rule
    does not admit the seam pairs and the edge pairs as written together. Where the last tile is
    padded (``rows % tile != 0``) the edge pairs are taken as written and the seam moves out by the
    smallest step that is free (``(n-3, n+1)``, ``(n+3, n-4)``); else the seam is taken as written and
    the edges move in (``(R-3, x)``, ``(x, R-4)``, ``(1, y)``)."""
    if rows % 2 or rows < 64 or tile < 16 or blocks < 1:
        raise ValueError("boundary_probes: need an even row count >= 64, tile >= 16, blocks >= 1")
    pl = _ProbePlacer(rows, tile, blocks, cross_view)
    for b in range(blocks):
        o = b * rows
        # (the one order that matters: the seam and edge pairs exclude each other, see above)
        for category in ((_edge_probes, _seam_probes) if rows % tile else (_seam_probes, _edge_probes)):
            category(pl, o)
        _self_mask_probes(pl, o)
        _positive_probes(pl, o)
        _corner_probes(pl, o)
    if blocks > 1:
        for a in range(blocks if blocks > 2 else 1):  # each block with the next (two blocks: one pair)
            (_cross_block_xview_probes if cross_view else _cross_block_probes)(pl, a * rows, (a + 1) % blocks * rows)
    return (pl.probes, pl.labels) if return_labels else pl.probes


class _ProbePlacer:
    """The probe list under construction and its rules: ``put`` takes the first candidate of a
    category whose rows are in range, are a (row, negative) pair, cross-view if asked, and neither
    probe rows nor positives of probe rows already."""

    def __init__(self, rows: int, tile: int, blocks: int, cross_view: bool):
        self.R, self.n, self.t, self.blocks, self.cross_view = rows, rows // 2, tile, blocks, cross_view
        # cross-view: the tiles are those of the N x N block Z1 Z2^T
        self.lim = self.n if cross_view else rows
        self.ntile = (self.lim + tile - 1) // tile
        self.last = (self.ntile - 1) * tile  # first row of the last tile
        self.taken, self.probes, self.labels = set(), [], []

    def pos(self, k: int) -> int:
        b, l = divmod(k, self.R)
        return b * self.R + (l + self.n) % self.R

    def free(self, i: int, j: int, cross_block: bool = False) -> bool:
        total = self.blocks * self.R
        if not (0 <= i < total and 0 <= j < total) or i == j or j == self.pos(i):
            return False
        if self.cross_view and ((i // self.R != j // self.R) != cross_block
                                or (i % self.R >= self.n) == (j % self.R >= self.n)):
            return False
        return i not in self.taken and j not in self.taken

    def put(self, label, cands, cross_block: bool = False) -> bool:
        for i, j in cands:
            if self.free(i, j, cross_block):
                self.taken.update((i, j, self.pos(i), self.pos(j)))
                self.probes.append((i, j))
                self.labels.append(label)
                return True
        return False


def _seam_probes(pl: _ProbePlacer, o: int) -> None:
    n = pl.n
    pl.put(("seam",), [(o + n - 1, o + n), (o + n - 3, o + n + 1)])
    pl.put(("seam",), [(o + n + 2, o + n - 2), (o + n + 3, o + n - 4)])


def _edge_probes(pl: _ProbePlacer, o: int) -> None:
    """First and last valid rows and columns; the partners are view-1 rows from the middle of the
    view, away from every edge (the first row's partner is the same row of view 2)."""
    R, n = pl.R, pl.n
    xs = [o + n // 2 + x for x in (7, 11, 13, 19, 23, 29)]
    pl.put(("last-row",), [(o + r, x) for r in (R - 1, R - 3) for x in xs])
    pl.put(("last-col",), [(x, o + c) for c in (R - 2, R - 4) for x in xs])
    pl.put(("first-row",), [(o + r, x + n) for r in (0, 1) for x in xs])


def _self_mask_probes(pl: _ProbePlacer, o: int) -> None:
    """``(m-1, m)`` and ``(m+2, m+1)`` at the first free m of each kind of multiple (cross-view: the
    same elements of the N x N block, which lie beside the positive). Both or neither are placed."""
    t, lim, last = pl.t, pl.lim, pl.last
    groups = [(("@last",) if last > t else ("@last", "@tile"), [last] if last > 0 else []),
              (("@tile",), list(range(t, last, t))),
              (("@64",), [m for m in range(64, lim - 2, 64) if m % t]),
              (("@16",), [m for m in range(16, lim - 2, 16) if m % 64 and m % t])]
    for tags, ms in groups:
        if t == 64 and "@tile" in tags:
            tags = tags + ("@64",)
        for m in ms:
            if pl.cross_view:
                up, lo = (o + m - 1, pl.pos(o + m)), (pl.pos(o + m + 2), o + m + 1)
            else:
                up, lo = (o + m - 1, o + m), (o + m + 2, o + m + 1)
            if m + 2 < lim and pl.free(*up) and pl.free(*lo):
                pl.put(("self-up",) + tags, [up])
                pl.put(("self-lo",) + tags, [lo])
                break


def _positive_probes(pl: _ProbePlacer, o: int) -> None:
    """``(a, p(a)+1)`` and ``(a', p(a')-1)`` with a, a' in the first, a middle and the last tile, a few
    rows into the tile (any free row of the tile will do: the candidates are tried in turn).
    Cross-view: every other tile's rows come from view 2, so both directions occur."""
    t, lim = pl.t, pl.lim
    for k, T0 in enumerate(sorted({0, pl.ntile // 2, pl.ntile - 1})):
        offs = [x for x in (5, 21, 9, 37, 45, 53, 11, 27) if T0 * t + x < min((T0 + 1) * t, lim)]
        a0 = o + T0 * t + (pl.n if pl.cross_view and k % 2 else 0)
        pl.put(("pos+1",), [(a0 + x, pl.pos(a0 + x) + 1) for x in offs])
        pl.put(("pos-1",), [(a0 + x, pl.pos(a0 + x) - 1) for x in reversed(offs)])


def _corner_probes(pl: _ProbePlacer, o: int) -> None:
    """The two corners of the off-diagonal tile (first tile, last tile) and of its mirror, each the
    first free element stepping diagonally into the tile from the corner."""
    if pl.ntile < 2:
        return
    co = o + pl.n if pl.cross_view else o  # columns of the tile; its mirror swaps the roles
    r1, c0, c1 = pl.t - 1, pl.last, pl.lim - 1
    pl.put(("corner-up",), [(o + s, co + c1 - s) for s in range(1, 12)])
    pl.put(("corner-up",), [(o + r1 - s, co + c0 + s) for s in range(3, 14)])
    pl.put(("corner-lo",), [(co + c0 + 5 + s, o + r1 - 5 - s) for s in range(12)])
    pl.put(("corner-lo",), [(co + c1 - 5 - s, o + 5 + s) for s in range(12)])


def _cross_block_probes(pl: _ProbePlacer, oa: int, ob: int) -> None:
    """Pairs with one row in the block at ``oa`` and one in the block at ``ob``."""
    R, t = pl.R, pl.t
    pl.put(("cross-block", "upper"), [(oa + 8 + s, ob + R - 9 - s) for s in range(16)])
    pl.put(("cross-block", "upper"), [(oa + t - 9 - s, ob + 8 + s) for s in range(16)])
    pl.put(("cross-block", "mirror"), [(ob + 24 + s, oa + t - 25 - s) for s in range(16)])
    pl.put(("cross-block", "mirror"), [(ob + R - 25 - s, oa + 24 + s) for s in range(16)])
    pl.put(("cross-block", "boundary"), [(oa + R - 5 - s, ob + 64 + s) for s in range(12)])


def _cross_block_xview_probes(pl: _ProbePlacer, oa: int, ob: int) -> None:
    """Cross-view pairs with the row in one block and the column in the other, both directions; local
    indices count within a view. Rows from the middle of the view, tried in turn (a candidate list
    like any other here; with it the seeded inputs of tests/test_infonce_dist_cpu.py keep the input
    conditions sig >= 0.2 and 0.15 <= P_ij <= 0.85, which a row with an unusually strong positive breaks)."""
    n = pl.n
    ls = [x for x in (100, 70, 43, 23, 55, 85, 115, 33, 63, 93, 48, 78, 108) if 1 <= x < n - 1]
    for d, (oi, oj) in enumerate(((oa, ob), (ob, oa))):
        kinds = [("would-be", [(l, l) for l in ls]), ("pos+1", [(l, l + 1) for l in ls]),
                 ("pos-1", [(l, l - 1) for l in ls]),
                 ("last-col", [(l, c) for c in range(n - 1, n - 17, -1) for l in ls]),
                 ("first-col", [(l, c) for c in range(16) for l in ls])]
        for k, (name, cands) in enumerate(kinds):
            v = (k + d) % 2  # the view of row i: both sides occur in both directions
            pl.put(("cross-block", name), [(oi + v * n + l, oj + (1 - v) * n + c) for l, c in cands], cross_block=True)


def plant_pairs(h: torch.Tensor, probes: Sequence[Tuple[int, int]], c: float) -> torch.Tensor:
    """A copy of ``h`` in which row j of every probe (i, j) is ``|h_j| (c u_i + sqrt(1 - c^2) r)``,
    ``u_i = h_i / |h_i|`` and r the unit part of the old h_j orthogonal to h_i: ``cos_ij = c`` exactly,
    the norm of row j unchanged. The probes must keep the rules of ``boundary_probes`` (no j is
    another probe's row)."""
    if not 0.0 < c < 1.0:
        raise ValueError("plant_pairs: need 0 < c < 1")
    out = h.clone()
    for i, j in probes:
        u = h[i] / h[i].norm()
        r = h[j] - (h[j] @ u) * u
        out[j] = h[j].norm() * (c * u + math.sqrt(1.0 - c * c) * r / r.norm())
    return out


def probe_signatures(h: torch.Tensor, temperature: float, probes: Sequence[Tuple[int, int]], *,
                     grad: Optional[torch.Tensor] = None, cross_view: bool = False):
    """(sig [k, 2], P [k]) in the dtype of ``h`` (use fp64): for probe (i, j), ``sig[:, 0]`` is the
    share of row i's gradient that the single element (i, j) carries,

        sig(a, b) = max| inv_a (P_ab + P_ba) / (R tau) (z_b - (z_a . z_b) z_a) | / max|grad_a|,

    ``sig[:, 1]`` is sig(j, i), and ``P`` is P_ij, the softmax weight of column j in row i.
    ``grad`` is dL/dh of the loss (computed here when not given); ``cross_view`` takes the softmax
    of cross-view InfoNCE."""
    R = h.shape[0]
    tau = float(temperature)
    if grad is None:
        grad = (info_nce_backward_analytic if cross_view else ntxent_backward_analytic)(h, tau)
    z, inv = normalize(h)
    ii = torch.tensor([p[0] for p in probes], device=h.device)
    jj = torch.tensor([p[1] for p in probes], device=h.device)
    rows = torch.cat([ii, jj])
    S = z[rows] @ z.t() / tau  # only the probe rows of the square
    col = torch.arange(R, device=h.device)
    if cross_view:
        S = S.masked_fill((rows >= R // 2).unsqueeze(1) == (col >= R // 2).unsqueeze(0), float("-inf"))
    else:
        S = S.masked_fill(rows.unsqueeze(1) == col.unsqueeze(0), float("-inf"))
    P = torch.exp(S - torch.logsumexp(S, dim=1, keepdim=True))
    k = len(probes)
    ar = torch.arange(k, device=h.device)
    p_ij, p_ji = P[ar, jj], P[k + ar, ii]

    def sig(a, b):
        cos = (z[a] * z[b]).sum(1, keepdim=True)
        part = inv[a].unsqueeze(1) * ((p_ij + p_ji) / (R * tau)).unsqueeze(1) * (z[b] - cos * z[a])
        return part.abs().max(1).values / grad[a].abs().max(1).values

    return torch.stack([sig(ii, jj), sig(jj, ii)], 1), p_ij


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
