"""Planted-pair probes through every similarity path of the project, on an MI355X.

The other GPU parity tests measure the gradient error against the global max|g| on random data and
cannot see an error in one element of the 2N x 2N square (tests/test_probes_cpu.py shows it with an
fp64 model). Here every case runs the public op ONCE on an input in which each probe (i, j) of
ops/reference.py boundary_probes carries at least sig_min >= 0.2 of the gradients of rows i and j
(elements beside the self and positive masks, at the seam of the views, on the first and last valid
rows and columns, in the corners of an upper tile and of its mirror, across ranks), and compares rows
i and j, each against its own max, with an fp64 oracle computed on the GPU:

    err_r = max|dh_r - ref_r| / max|ref_r|        for both rows of every probe

An element that is dropped, misplaced or counted twice moves err by about the signature, two orders
above the bounds below. Each case first asserts from the host planning bindings that its shape takes
the path it names on this machine's CU count. Inputs, probe lists and c: tests/test_probes_cpu.py
CASES (the same fp64 inputs, rounded to the input dtype here).

Bounds. Per-row: 2 x the largest per-row error measured on MI355X over all cases of the compute
dtype (ROW_MEASURED), which must also stay under sig_min / 4 of every case (the test computes
sig_min itself). Loss and global gradient error: 2 x max(tests/test_gpu_kernels.py TOL, measured
here), per family of paths (MEASURED). On this unsaturated data (loss 0.5 .. 2.4) the 16-bit loss errors
are 1e-5 .. 1.4e-4, above the table's 1.2e-6 / 7e-7, which were measured on saturated data (loss
0.0025); the gradient errors all stay under the table. Measured largest per-row errors: fp32 5.5e-6,
fp16 5.0e-3, bf16 1.8e-2, against caps sig_min / 4 of 5.8e-2 .. 1.1e-1 ("Planted-pair
probes"); every case prints its own figures in one `PROBE` line.
Reference intent: the reference's gradient tests (tests/test_backward.cpp), element by element.
"""
import functools
import math

import pytest
import torch

from ntxent_amd.ops import reference as R
from test_probes_cpu import CASES, TAU, probe_case, row_errors

pytestmark = pytest.mark.gpu

# tests/test_gpu_kernels.py TOL: (loss rel err, grad max-abs err / global max|g|)
TABLE = {"fp32": (2e-9, 6e-6), "fp16": (1.2e-6, 8e-3), "bf16": (7e-7, 2.2e-2)}
# largest per-row error of a probe row over all cases of the compute dtype, measured on MI355X
# (fp32 5.46e-6 at 6144 x 2048 stream-K; fp16 5.00e-3 and bf16 1.83e-2 at 1000 x 2048 split-K forward, both
# with bf16 rows in and a bf16 gradient out, whose own rounding is 2^-9 of each element; with fp32
# rows the 16-bit cases stay under 3.3e-3 (emulated ranks, W = 3 x 300 rows all-gather) and 5.5e-3 (InfoNCE bf16))
ROW_MEASURED = {"fp32": 5.46e-6, "fp16": 5.00e-3, "bf16": 1.83e-2}
# largest (loss rel err, global grad err) per family of paths and compute, measured on MI355X
MEASURED = {
    "small": {"fp16": (2.01e-6, 3.28e-3), "bf16": (1.41e-4, 6.44e-3)},
    "large": {"fp32": (1.38e-7, 5.02e-6), "fp16": (9.58e-6, 4.18e-3), "bf16": (6.19e-5, 9.94e-3)},
    "ranks": {"fp32": (5.28e-8, 1.48e-6), "fp16": (1.61e-5, 1.26e-3)},
    "xview": {"fp32": (1.62e-7, 1.37e-6), "fp16": (1.31e-5, 3.67e-4), "bf16": (1.21e-4, 3.30e-3)},
}
IN_DTYPE = {"fp16": torch.bfloat16, "bf16": torch.bfloat16, "fp32": torch.float32}
COMPUTES3 = ["fp16", "bf16", "fp32"]


@functools.lru_cache(maxsize=2)
def _oracle(name, in_dtype):
    """(device input, fp64 loss, fp64 gradient, sig_min) of a case: the fp64 oracle of the rounded
    input, on the GPU, shared by the tests of that case."""
    h64, probes, _, _ = probe_case(name)
    xview = CASES[name][4]
    h = h64.to(in_dtype).cuda()
    x = h.double().requires_grad_(True)
    loss = (R.info_nce_loss if xview else R.ntxent_loss)(x, TAU)
    (g,) = torch.autograd.grad(loss, x)
    sig, p_ij = R.probe_signatures(x.detach(), TAU, probes, grad=g, cross_view=xview)
    assert sig.min().item() >= 0.2 and 0.15 <= p_ij.min().item() and p_ij.max().item() <= 0.85
    return h, loss.item(), g, sig.min().item()


def _check(tag, family, name, compute, loss, grad):
    """Finite results, the per-row bound on every probe row (under its sig_min / 4 cap), and the loss
    and global gradient bounds; prints the case's figures first."""
    in_dtype = IN_DTYPE[compute] if family in ("small", "large") else torch.float32  # (the others: fp32 rows)
    _, lref, gref, sig_min = _oracle(name, in_dtype)
    _, probes, labels, _ = probe_case(name)
    assert math.isfinite(loss) and torch.isfinite(grad).all()
    rerr = row_errors(grad, gref, probes)
    lerr = abs(loss - lref) / max(1.0, abs(lref))
    gerr = (grad.double() - gref).abs().max().item() / gref.abs().max().item()
    k = rerr.amax(1).argmax().item()
    bound = 2.0 * ROW_MEASURED[compute]
    lt, gt = (2.0 * max(t, m) for t, m in zip(TABLE[compute], MEASURED[family][compute]))
    print(f"PROBE {tag} case={name} compute={compute} probes={len(probes)} sig_min={sig_min:.3f} "
          f"row_err_max={rerr.max().item():.3e} at={probes[k]}{'/'.join(labels[k])} bound={bound:.3e} cap={sig_min / 4:.3e} "
          f"loss_err={lerr:.3e} (bound {lt:.1e}) grad_err={gerr:.3e} (bound {gt:.1e})")
    assert bound <= sig_min / 4, (bound, sig_min)
    bad = [(probes[i], labels[i], [f"{e:.2e}" for e in rerr[i].tolist()]) for i in range(len(probes))
           if rerr[i].max().item() > bound]
    assert not bad, f"probe rows over the per-row bound {bound:.2e}: {bad}"
    assert lerr <= lt, (lerr, lt)
    assert gerr <= gt, (gerr, gt)


def _op(name, compute, keep=True):
    import ntxent_amd

    h = _oracle(name, IN_DTYPE[compute])[0]
    x = h.clone().requires_grad_(True)
    loss = ntxent_amd.ntxent_loss(x, TAU, compute=compute, keep_logits=keep)
    (g,) = torch.autograd.grad(loss, x)
    torch.cuda.synchronize()
    return loss.item(), g


def _plan(ext, name, compute, keep=True):
    """(step plan, forward K-steps per tile, row tiles, CU count) of a case as the op resolves it."""
    rows, dim = CASES[name][:2]
    cus = ext.device_info(0)["num_cus"]
    inp = {torch.bfloat16: "bf16", torch.float32: "fp32"}[IN_DTYPE[compute]]
    plan = ext.step_plan(rows, dim, inp, compute, keep, cus)
    g = ext.geometry(rows, dim)
    nk = g["dim_k"] * (4 if compute == "fp32" else 2) // ext.K_STEP_BYTES
    return plan, nk, g["row_tiles"], cus


# ---- the small path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["fp16", "bf16"])
@pytest.mark.parametrize("name,fused,splits", [("small-600x200", True, 0), ("small-600x200", True, 1),
                                               ("small-600x200", True, 3), ("small-1500x96", False, 0)])
def test_small_path(ext, name, fused, splits, compute):
    """One forward and one backward launch (small_kernels.hip, 64-row tiles): the fused row prologue
    and the separate one, the backward's column splits 1, 3 and the default 8."""
    try:
        ext.set_small_splits(splits)
        plan, _, _, _ = _plan(ext, name, compute)
        assert plan["small"] and plan["small_fwd_fused"] == fused
        assert plan["small_splits"] == (splits or 8)
        loss, g = _op(name, compute)
    finally:
        ext.set_small_splits(0)
    _check(f"small splits={splits or 8}", "small", name, compute, loss, g)


# ---- the large pipeline and its forward schedules ---------------------------------------------------
@pytest.mark.parametrize("compute", COMPUTES3)
@pytest.mark.parametrize("name", ["large-600x320", "large-600x300"])
def test_large_pipeline_at_small_size(ext, name, compute):
    """The 256-row-tile pipeline with padded rows (600 = 2 tiles + 88) and d % 64 != 0; d = 300 is
    not a multiple of 8 either, so the normalisation backward is its own launch (not fuse)."""
    plan, _, _, _ = _plan(ext, name, compute)
    assert not plan["small"] and not plan["raw"] and plan["keep_cos"]
    assert plan["fuse"] == (compute != "fp32" and name == "large-600x320")
    _check("large", "large", name, compute, *_op(name, compute))


@pytest.mark.parametrize("compute", COMPUTES3)
def test_splitk_forward_padded_rows(ext, compute):
    plan, nk, rt, cus = _plan(ext, "large-1000x2048", compute)
    assert not plan["small"] and ext.fwd_splitk_pieces(plan["n_own"], nk, cus, rt) >= 2
    _check("splitk-fwd", "large", "large-1000x2048", compute, *_op("large-1000x2048", compute))


@pytest.mark.parametrize("compute", COMPUTES3)
def test_diagonal_remainder_with_padded_last_tile(ext, compute):
    """5800 rows = 23 panels, 276 own tiles: one whole round on 256 CUs and a remainder of 20 diagonal
    tiles (the list ends with the diagonal tiles in panel order), the last of them padded (5800 =
    22 x 256 + 168); unit rows, not the raw forward."""
    plan, nk, rt, cus = _plan(ext, "large-5800x256", compute)
    assert ext.fwd_diag_remainder(plan["n_own"], nk, cus, rt) > 0 and not plan["raw"] and CASES["large-5800x256"][0] % 256
    _check("diag-remainder", "large", "large-5800x256", compute, *_op("large-5800x256", compute))


@pytest.mark.parametrize("compute", COMPUTES3)
def test_stream_k_forward_remainder(ext, compute):
    """6144 x 2048: 300 own tiles = one round + 44 tiles that are not all diagonal, split over the
    grid in K pieces (stream-K), each tile finished by its last arriver."""
    plan, nk, rt, cus = _plan(ext, "large-6144x2048", compute)
    assert ext.fwd_diag_remainder(plan["n_own"], nk, cus, rt) == 0
    assert ext.fwd_splitk_pieces(plan["n_own"], nk, cus, rt) == 0
    s = ext.schedule(plan["n_own"], nk, cus)
    assert s["sk_tiles"] > 0 and s["dp_tiles"] > 0 and s["ipb"] < nk  # more than one piece per tile
    _check("stream-k", "large", "large-6144x2048", compute, *_op("large-6144x2048", compute))


@pytest.mark.parametrize("compute", ["fp16", "bf16"])
def test_raw_forward_lse_fold_half_c_splitk_dz_dot_fold(ext, compute):
    """8192 x 256: raw-operand forward, a diagonal remainder of exactly the second half's panels (so
    the LSE launch folds into it), half C, a split-K dZ whose reduce takes the folded dot. With the
    dot fold's poll disabled every epilogue sums its rows' dot itself: the same additions, so the
    same bits."""
    name = "large-8192x256"
    _assert_8192x256_path(ext, compute)
    loss, g = _op(name, compute)
    spin = ext.dot_fold_spin()
    try:
        ext.set_dot_fold_spin(0)
        loss_nospin, g_nospin = _op(name, compute)
    finally:
        ext.set_dot_fold_spin(spin)
    _check("raw+fold+halfC", "large", name, compute, loss, g)
    _check("raw+fold+halfC spin=0", "large", name, compute, loss_nospin, g_nospin)
    assert loss_nospin == loss and torch.equal(g_nospin, g)


def _assert_8192x256_path(ext, compute):
    name = "large-8192x256"
    plan, nk, rt, cus = _plan(ext, name, compute)
    assert plan["raw"] and plan["half_c"] and plan["dfold"] and plan["fuse"]
    # the LSE fold: the remainder is exactly the diagonal tiles of the second half of the rows
    assert ext.lse_fold_enabled() and ext.fwd_diag_remainder(plan["n_own"], nk, cus, rt) * 256 == CASES[name][0] // 2
    assert ext.fwd_splitk_pieces(plan["n_dz"], CASES[name][0] * 2 // ext.K_STEP_BYTES, cus, 1) >= 3  # split-K dZ


@pytest.mark.parametrize("compute", ["fp16", "bf16"])
def test_lse_launch_instead_of_fold_same_bits(ext, compute):
    """The same step with set_lse_fold(False): the LSE launch merges the column-tile partials instead
    of the diagonal remainder's blocks, in the fold's order (each quarter of the column tiles in tile
    order, the quarters in order, the diagonal tile's partial of a second-half row last:
    RawRows::lse_fold_order), so the toggle moves the merge to another kernel and changes no bit.
    Before the launch took that order it merged 8 strided lanes in an xor tree; the loss was the same
    bits and 27 (fp16) / 30 (bf16) of the 2097152 gradient elements differed by one bf16 ulp
    (at most 1.2e-7). The probes are checked on this path as well."""
    name = "large-8192x256"
    _assert_8192x256_path(ext, compute)
    loss, g = _op(name, compute)
    try:
        ext.set_lse_fold(False)
        loss_nofold, g_nofold = _op(name, compute)
    finally:
        ext.set_lse_fold(True)
    _check("raw+LSE launch+halfC", "large", name, compute, loss_nofold, g_nofold)
    diff = (g_nofold.float() - g.float()).abs()
    print(f"PROBE lse_fold off vs on compute={compute}: loss diff {abs(loss_nofold - loss):.3e} grad elements that differ "
          f"{(diff > 0).sum().item()} of {diff.numel()} max diff {diff.max().item():.3e} max|g| {g.float().abs().max().item():.3e}")
    assert loss_nofold == loss and torch.equal(g_nofold, g)


@pytest.mark.parametrize("compute", ["fp16", "bf16"])
def test_whole_round_dz_with_half_c(ext, compute):
    plan, _, _, cus = _plan(ext, "large-8192x2048", compute)
    assert plan["half_c"] and plan["n_dz"] == 256
    _check("halfC whole-round dZ", "large", "large-8192x2048", compute, *_op("large-8192x2048", compute))


@pytest.mark.parametrize("compute", COMPUTES3)
@pytest.mark.parametrize("name", ["large-600x320", "large-5800x256"])
def test_recompute_coefficient_gemm(ext, name, compute):
    """keep_logits=False: the backward's coefficient GEMM recomputes the cosines from the unit rows."""
    plan, _, _, _ = _plan(ext, name, compute, keep=False)
    assert not plan["keep_cos"] and not plan["small"] and not plan["raw"] and not plan["half_c"]
    _check("recompute", "large", name, compute, *_op(name, compute, keep=False))


@pytest.mark.parametrize("compute", ["fp16", "bf16"])
def test_native_engine_step(ext, compute):
    """The native Engine issues the op's launch sequence (tests/test_gpu_step_shared.py): the same
    bits, and the same probes."""
    name = "large-8192x256"
    rows, dim = CASES[name][:2]
    _assert_8192x256_path(ext, compute)  # (the Engine resolves the same step plan)
    h = _oracle(name, torch.bfloat16)[0]
    eng = ext.NativeEngine(rows, dim, TAU, "bf16", compute)
    loss, dh = eng.step(h)
    torch.cuda.synchronize()
    loss, dh = loss.item(), dh.clone()
    del eng
    _check("engine", "large", name, compute, loss, dh)
    lo, go = _op(name, compute)
    assert loss == lo and torch.equal(dh, go)


# ---- the emulated W-rank drivers --------------------------------------------------------------------
def _drivers():
    from ntxent_amd.parallel import emulate

    return {"dist": emulate.emulated_dist_forward_backward, "sym": emulate.emulated_sym_forward_backward,
            "ring": emulate.emulated_ring_forward_backward}


@pytest.mark.parametrize("compute", ["fp16", "fp32"])
@pytest.mark.parametrize("driver", ["dist", "sym", "ring"])
@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("rows", [300, 600])
def test_emulated_ranks(ext, rows, W, driver, compute):
    """W virtual ranks of 300 rows (one tile + 44 rows, the last tile mostly padding) and, as an extra,
    of 600 rows (2 tiles + 88 rows) through the data-parallel stage ops: all-gather, symmetric and
    ring negatives. (With world > 1 no plan is small, so 300 rows take the 256-row-tile pipeline.) The probes are planted in the global pair order;
    their list is built for the rank-stacked rows, so every rank has the whole set at its own tile
    edges, and the cross-block pairs sit on two ranks: cross tiles and their mirrored coefficients."""
    name = f"ranks{W}-{rows}x320"
    n, N = rows // 2, W * rows // 2
    hg = _oracle(name, torch.float32)[0]
    shards = [torch.cat([hg[r * n:(r + 1) * n], hg[N + r * n:N + (r + 1) * n]], 0).contiguous() for r in range(W)]
    plans = [ext.get_plan(rows, CASES[name][1], W, r, TAU, compute, 0) for r in range(W)]
    assert all(p.world == W and not p.small and p.rows_pad > p.rows and p.col_tiles == W * p.row_tiles for p in plans)
    loss, grads = _drivers()[driver](shards, TAU, compute=compute)
    torch.cuda.synchronize()
    g = torch.cat([x[:n] for x in grads] + [x[n:] for x in grads], 0)  # back to the global pair order
    _check(f"emulated-{driver} W={W}", "ranks", name, compute, loss.item(), g)


# ---- cross-view InfoNCE -----------------------------------------------------------------------------
@pytest.mark.parametrize("compute", COMPUTES3)
@pytest.mark.parametrize("name", ["xview-400x100", "xview-400x256", "xview-768x100", "xview-768x256"])
def test_info_nce(gpu, name, compute):
    """N = 200 and 384 (128-row tiles of the N x N block: a padded last tile, and three whole ones):
    cross-view probes in both directions, beside the positive at the 16-, 64- and tile edges; four
    same-view decoys at cos 0.9 that the loss must not see."""
    import ntxent_amd

    h = _oracle(name, torch.float32)[0]
    x = h.clone().requires_grad_(True)
    loss = ntxent_amd.info_nce_loss(x, TAU, compute=compute)
    (g,) = torch.autograd.grad(loss, x)
    torch.cuda.synchronize()
    _check("info_nce", "xview", name, compute, loss.item(), g)
