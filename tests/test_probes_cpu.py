"""Planted-pair probes (ops/reference.py: boundary_probes, plant_pairs, probe_signatures), on the CPU.

The GPU parity tests measure the gradient error against the GLOBAL max|g| on random two-view data,
where one negative carries about 1/2N of a row's softmax mass: an error in one element of the
2N x 2N square stays far below the 16-bit tolerances (test_old_metric_cannot_see_one_element). A
probe (i, j) plants cos_ij = c so that the single element (i, j) carries a known share, the
signature, of the gradients of rows i and j; tests/test_gpu_probes.py then measures the error per
probe row. This file checks the harness itself: the structure of the probe lists, the planting, the
input conditions at every shape the GPU file runs (CASES, shared with it), and, with an fp64 model of
the step, that a fault in one element moves the per-row metric by more than half the signature.
Reference intent: the gradient of the reference's backward (src/ntxent_kernel.cu:232-262), element by element.
"""
import functools
import math

import pytest
import torch

from ntxent_amd.ops import reference as R

TAU = 0.07

# Every input of tests/test_gpu_probes.py: name -> (rows of one block, dim, tile edge of the path,
# blocks, cross_view, c). c = None takes the rule c = min(0.9, tau ln(2R)), R the row count of the
# whole batch. Where the rule leaves this file's seeded data outside the input conditions
# (sig_min >= 0.2, 0.15 <= P_ij <= 0.85) the case names its own c: the conditions stay.
CASES = {
    "small-600x200": (600, 200, 64, 1, False, None),
    "small-1500x96": (1500, 96, 64, 1, False, 0.62),
    "large-600x320": (600, 320, 256, 1, False, None),
    "large-600x300": (600, 300, 256, 1, False, None),
    "large-1000x2048": (1000, 2048, 256, 1, False, None),
    "large-5800x256": (5800, 256, 256, 1, False, None),
    "large-6144x2048": (6144, 2048, 256, 1, False, None),
    "large-8192x256": (8192, 256, 256, 1, False, None),
    "large-8192x2048": (8192, 2048, 256, 1, False, None),
    "ranks2-300x320": (300, 320, 256, 2, False, None),  # 300 rows per rank: one tile + 44 rows
    "ranks3-300x320": (300, 320, 256, 3, False, None),
    "ranks2-600x320": (600, 320, 256, 2, False, None),  # (extra: two tiles + 88 rows per rank)
    "ranks3-600x320": (600, 320, 256, 3, False, None),
    "xview-400x100": (400, 100, 128, 1, True, 0.55),
    "xview-400x256": (400, 256, 128, 1, True, 0.55),
    "xview-768x100": (768, 100, 128, 1, True, 0.55),
    "xview-768x256": (768, 256, 128, 1, True, 0.55),
}


def two_views(rows, dim, seed):
    """Unsaturated two-view data: base + 1.0 * noise per view, fp64."""
    g = torch.Generator().manual_seed(seed)
    n = rows // 2
    base = torch.randn(n, dim, generator=g, dtype=torch.float64)
    return torch.cat([base + torch.randn(n, dim, generator=g, dtype=torch.float64),
                      base + torch.randn(n, dim, generator=g, dtype=torch.float64)], 0)


def decoys(rows, probes, count=4):
    """Same-view pairs (cross-view InfoNCE masks them) of rows no probe uses, first view 1 then 2."""
    n = rows // 2
    busy = {k for p in probes for k in p} | {(k + n) % rows for p in probes for k in p}
    out = []
    for lo in (0, n):
        free = [k for k in range(lo + 30, lo + n - 1) if k not in busy]
        for _ in range(count // 2):
            i, j = free.pop(0), free.pop(0)
            busy.update((i, j, (i + n) % rows, (j + n) % rows))
            free = [k for k in free if k not in busy]
            out.append((i, j))
    return out


@functools.lru_cache(maxsize=None)
def probe_case(name):
    """(planted fp64 input, probes, labels, c) of a case. With blocks > 1 the input is in
    global_pair_order and the probe indices are mapped into it (the list is built for the
    rank-stacked rows, whose tiles the kernels index). Cross-view cases also get four same-view
    decoys planted at c = 0.9."""
    rows, dim, tile, blocks, xview, c = CASES[name]
    probes, labels = R.boundary_probes(rows, tile, blocks=blocks, cross_view=xview, return_labels=True)
    total = rows * blocks
    if c is None:
        c = min(0.9, TAU * math.log(2 * total))
    if blocks > 1:
        m = R.stacked_to_pair_order(blocks, rows).tolist()
        probes = [(m[i], m[j]) for i, j in probes]
        h = R.global_pair_order([two_views(rows, dim, seed=rows + dim + 101 * r) for r in range(blocks)])
    else:
        h = two_views(rows, dim, seed=rows + dim)
    h = R.plant_pairs(h, probes, c)
    if xview:
        h = R.plant_pairs(h, decoys(rows, probes), 0.9)
    return h, probes, labels, c


def row_errors(got, ref, probes):
    """The per-row metric: err_r = max|got_r - ref_r| / max|ref_r| for rows i and j of every probe,
    a [k, 2] tensor."""
    idx = torch.tensor(probes, device=ref.device)
    return (got[idx].double() - ref[idx]).abs().amax(2) / ref[idx].abs().amax(2)


# ---- the probe list ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_probe_list_rules_and_categories(name):
    rows, _, tile, blocks, xview, _ = CASES[name]
    probes, labels = R.boundary_probes(rows, tile, blocks=blocks, cross_view=xview, return_labels=True)
    assert probes == R.boundary_probes(rows, tile, blocks=blocks, cross_view=xview)
    n, total = rows // 2, rows * blocks

    def pos(k):
        return k // rows * rows + (k % rows + n) % rows

    assert len(probes) >= 16
    used = [k for p in probes for k in p]
    assert all(0 <= k < total for k in used)
    assert len(set(used)) == len(used)  # every row in at most one probe
    assert not {i for i, _ in probes} & {j for _, j in probes}  # no i is another probe's j
    assert not {pos(k) for k in used} & set(used)  # no probe row is the positive of a probe row
    assert all(j != i and j != pos(i) for i, j in probes)  # j is a negative of i
    if xview:  # both directions, cross-view only
        assert all((i % rows >= n) != (j % rows >= n) for i, j in probes)
        assert {i >= n for i, _ in probes} == {True, False}
    # categories, per block
    lim = n if xview else rows
    for b in range(blocks):
        mine = [(p, l) for p, l in zip(probes, labels) if p[0] // rows == b and "cross-block" not in l]
        have = lambda *tags: [p for p, l in mine if all(t in l for t in tags)]
        for side in ("self-up", "self-lo"):
            for at in ("@16", "@64", "@tile", "@last"):
                assert have(side, at), (b, side, at)
        o = b * rows
        for (i, j) in have("self-up"):
            assert (j == pos(i + 1) if xview else j == i + 1) and (i + 1 - o) % 16 == 0
        for (i, j) in have("self-lo"):
            assert (j == pos(i) - 1 if xview else j == i - 1) and (j - 1 - o) % 16 == 0
        assert any((i + 1 - o) == (lim - 1) // tile * tile for i, _ in have("self-up", "@last"))
        up, dn = have("pos+1"), have("pos-1")
        assert all(j == pos(i) + 1 for i, j in up) and all(j == pos(i) - 1 for i, j in dn)
        assert len({(i % rows % lim) // tile for i, _ in up}) >= min(3, (lim + tile - 1) // tile)
        assert len({(i % rows % lim) // tile for i, _ in dn}) >= min(3, (lim + tile - 1) // tile)
        seam = have("seam")
        assert len(seam) == 2 and all((i % rows < n) != (j % rows < n) and abs(i - j) <= 7 for i, j in seam)
        (lr,), (lc,), (fr,) = have("last-row"), have("last-col"), have("first-row")
        if rows % tile:  # a padded last tile: the edge pairs exactly as the issue writes them
            assert lr[0] == o + rows - 1 and lc[1] == o + rows - 2 and fr[0] == o
        else:  # the seam as written, the edges moved in by two rows
            assert set(seam) == {(o + n - 1, o + n), (o + n + 2, o + n - 2)}
            assert lr[0] == o + rows - 3 and lc[1] == o + rows - 4 and fr[0] == o + 1
        cu, cl = have("corner-up"), have("corner-lo")
        assert len(cu) == 2 and len(cl) == 2
        col = (lambda k: k % rows - n) if xview else (lambda k: k % rows)  # cross-view: block coordinates
        row = (lambda k: k % rows % n) if xview else (lambda k: k % rows)
        assert all(row(i) // tile < col(j) // tile for i, j in cu)  # the upper tile (I, J), I < J
        assert all(col(i) // tile > row(j) // tile for i, j in cl)  # its mirror (J, I)
        # first row with last column, last row with first column; and the same corners of the mirror
        assert any(row(i) < 16 and col(j) >= lim - 16 for i, j in cu)
        assert any(row(i) % tile >= tile - 16 and col(j) % tile < 16 for i, j in cu)
        assert any(col(i) >= lim - 16 and row(j) < 16 for i, j in cl)
        assert any(col(i) % tile < 16 and row(j) % tile >= tile - 16 for i, j in cl)
    if blocks > 1:
        cross = [p for p, l in zip(probes, labels) if "cross-block" in l]
        assert len(cross) >= 5 * (blocks if blocks > 2 else 1) and all(i // rows != j // rows for i, j in cross)
        assert {i // rows < j // rows for i, j in cross} == {True, False}  # cross tiles and their mirrors


def test_padded_and_unpadded_shapes_occur_per_path():
    for tile in (64, 128, 256):
        mods = {(rows if not xv else rows // 2) % t != 0 for rows, _, t, _, xv, _ in CASES.values() if t == tile}
        assert True in mods, tile


# ---- planting and the input conditions --------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_planting_and_input_conditions(name):
    rows, dim, _, blocks, xview, _ = CASES[name]
    h, probes, _, c = probe_case(name)
    assert h.dtype == torch.float64 and h.shape == (rows * blocks, dim)
    z, _ = R.normalize(h)
    ii, jj = torch.tensor(probes).t()
    assert ((z[ii] * z[jj]).sum(1) - c).abs().max().item() <= 1e-12
    sig, p_ij = R.probe_signatures(h, TAU, probes, cross_view=xview)
    loss = (R.info_nce_loss if xview else R.ntxent_loss)(h, TAU).item()
    print(f"PROBECPU {name} probes={len(probes)} c={c:.3f} loss={loss:.2f} P_ij={p_ij.min():.2f}..{p_ij.max():.2f} "
          f"sig_min={sig.min():.3f}")
    assert sig.min().item() >= 0.2
    assert 0.15 <= p_ij.min().item() and p_ij.max().item() <= 0.85


def test_plant_pairs_keeps_norms_and_other_rows():
    h = two_views(600, 200, seed=1)
    probes = R.boundary_probes(600, 64)
    hp = R.plant_pairs(h, probes, 0.5)
    planted = torch.tensor([j for _, j in probes])
    keep = torch.ones(600, dtype=torch.bool)
    keep[planted] = False
    assert torch.equal(hp[keep], h[keep])
    assert (hp[planted].norm(dim=1) - h[planted].norm(dim=1)).abs().max().item() <= 1e-12


def test_signature_is_the_elements_share_of_the_gradient():
    """Zeroing the coefficient C_ij (and its mirror C_ji) changes rows i and j by exactly the vector
    whose max-abs the signature reports."""
    h, probes, _, _ = probe_case("small-600x200")
    ref = R.ntxent_backward_analytic(h, TAU)
    sig, _ = R.probe_signatures(h, TAU, probes, grad=ref)
    for k in (0, 5, len(probes) - 1):
        i, j = probes[k]
        got = _step_model(h, TAU, ("drop2", i, j))
        err = row_errors(got, ref, [probes[k]])[0]
        assert abs(err[0].item() - sig[k, 0].item()) <= 1e-9 and abs(err[1].item() - sig[k, 1].item()) <= 1e-9


# ---- a test of the test: an fp64 model of the step with a fault in one element ----------------------
def _step_model(h, tau, fault=None):
    """The one-GPU step in fp64 (unit rows, LSE, C = P + P^T - 2 I_pos, dZ = C Z, normalisation
    backward), the same operations in the same order as R.ntxent_backward_analytic, so that the
    clean model equals it bit for bit. fault = (kind, i, j):
      "lse"   column j left out of row i's LSE;
      "drop"  the coefficient C[i, j] dropped;
      "swap"  C[i, j] and C[i, j'] swapped, j' the next column that is a negative of i;
      "drop2" C[i, j] and C[j, i] dropped (the element and its mirror)."""
    Rr = h.shape[0]
    z, inv = R.normalize(h)
    S = R.logits(h, tau)
    kind, i, j = fault or (None, 0, 0)
    if kind == "lse":
        Sx = S.clone()
        Sx[i, j] = float("-inf")
        lse = torch.logsumexp(Sx, dim=1)
    else:
        lse = torch.logsumexp(S, dim=1)
    P = torch.exp(S - lse.unsqueeze(1))
    pos = R.positive_index(Rr, h.device)
    C = P + P.t()
    C[torch.arange(Rr, device=h.device), pos] -= 2.0
    if kind in ("drop", "drop2"):
        C[i, j] = 0.0
        if kind == "drop2":
            C[j, i] = 0.0
    elif kind == "swap":
        j2 = next(k for k in (j + 1, j + 2, j - 1, j - 2) if 0 <= k < Rr and k != i and k != pos[i].item())
        C[i, j], C[i, j2] = C[i, j2].clone(), C[i, j].clone()
    dz = (C @ z) * (torch.as_tensor(1.0, dtype=h.dtype, device=h.device) / (Rr * tau))
    dot = (z * dz).sum(1, keepdim=True)
    return inv.unsqueeze(1) * (dz - z * dot)


@pytest.mark.parametrize("name", ["small-600x200", "large-600x320", "small-1500x96"])
def test_one_element_faults_move_the_per_row_metric(name):
    h, probes, _, _ = probe_case(name)
    ref = R.ntxent_backward_analytic(h, TAU)
    sig, _ = R.probe_signatures(h, TAU, probes, grad=ref)
    sig_min = sig.min().item()
    clean = row_errors(_step_model(h, TAU), ref, probes)
    assert clean.max().item() == 0.0
    worst = {}
    for kind in ("drop", "lse", "swap"):
        for k, (i, j) in enumerate(probes):
            err = row_errors(_step_model(h, TAU, (kind, i, j)), ref, [probes[k]])[0]
            assert err[0].item() > sig_min / 2, (kind, i, j, err.tolist(), sig_min)
            worst[kind] = min(worst.get(kind, 1e9), err[0].item())
    print(f"PROBEFAULT {name} sig_min={sig_min:.3f} smallest row-i error: " +
          " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


def test_old_metric_cannot_see_one_element():
    """The gap this harness closes. On the random data of the GPU parity tests (rows 1024, d 512,
    noise 0.3, seed 0, tau 0.07) a fault at one element of row 5, the negative of median weight
    (column 448, P = 2.0e-6 against a mean of 2.4e-6), stays four to two hundred times under the fp16
    tolerance of the global metric (8e-3 of max|g|, loss 1.2e-6: tests/test_gpu_kernels.py TOL): a
    dropped coefficient 1.2e-3, a column left out of the LSE 2.2e-4 (loss 2e-9), a swapped pair
    4.0e-5. Even at a heavy negative, column 300 with almost eight times the median weight, the three
    faults give 7.6e-3, 1.7e-3 and 1.1e-2 and pass the bf16 tolerance (2.2e-2). At a probe of the
    planted input a dropped coefficient moves the per-row metric by more than sig_min / 2, two
    orders above the clean 16-bit per-row errors."""
    g = torch.Generator().manual_seed(0)
    base = torch.randn(512, 512, generator=g, dtype=torch.float64)
    h = torch.cat([base + 0.3 * torch.randn(512, 512, generator=g, dtype=torch.float64),
                   base + 0.3 * torch.randn(512, 512, generator=g, dtype=torch.float64)], 0)
    ref = R.ntxent_backward_analytic(h, TAU)
    lref = R.ntxent_loss(h, TAU).item()
    S = R.logits(h, TAU)
    neg = torch.tensor([k for k in range(1024) if k not in (5, 5 + 512)])
    w = torch.softmax(S[5], 0)[neg]
    j = neg[(w - w.median()).abs().argmin()].item()  # the negative of median weight
    figures = {}
    for col, tol in ((j, 8e-3 / 4), (300, 2.2e-2)):
        for kind in ("drop", "lse", "swap"):
            got = _step_model(h, TAU, (kind, 5, col))
            gerr = (got - ref).abs().max().item() / ref.abs().max().item()
            figures[(col, kind)] = gerr
            assert 0.0 < gerr <= tol, (col, kind, gerr)  # wrong, and passed
    print("PROBEOLD " + " ".join(f"{c}/{k}={v:.2e}" for (c, k), v in figures.items()))
    Sx = S.clone()
    Sx[5, j] = float("-inf")
    pl = S.gather(1, R.positive_index(1024).unsqueeze(1)).squeeze(1)
    lerr = abs((torch.logsumexp(Sx, 1) - pl).mean().item() - lref) / max(1.0, lref)
    assert 0.0 < lerr <= 1.2e-6 / 100
    hp, probes, _, _ = probe_case("small-600x200")
    refp = R.ntxent_backward_analytic(hp, TAU)
    sig_min = R.probe_signatures(hp, TAU, probes, grad=refp)[0].min().item()
    i, j = probes[0]
    err = row_errors(_step_model(hp, TAU, ("drop", i, j)), refp, [probes[0]])[0, 0].item()
    assert err > sig_min / 2 >= 0.1
