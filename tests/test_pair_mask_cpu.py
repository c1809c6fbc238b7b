"""The NT-Xent pair rule of the kernels (csrc/kernels/pair_mask.h), checked exhaustively on the CPU.

Every kernel that masks, counts or weighs pairs inlines the header's functions; the `_C.pair_*`
bindings are thin host wrappers over the same functions. They are compared here, for every element
of the padded square, with a brute-force definition written out below and with ops/reference.py's
positive index:

  element (i, j) of the own block is a negative unless j == i, j == p(i), or i or j is padding.

The conservative pre-tests (window_plain, tile_near, fragment_near) have one-sided contracts:
soundness is checked for every window / tile / fragment, and usefulness (the test is not
constantly on the safe side) where the issue of a constant answer would go unseen.
"""
import numpy as np
import pytest

from ntxent_amd.ops import reference as R_

ROWS = [6, 130, 600, 1000]
TILE = 256


def _rpad(R):
    return (R + TILE - 1) // TILE * TILE


def _brute(R, n):
    """(special, selfpos) [n][n] bool: no negative / self or positive, by the definition."""
    pos = R_.positive_index(R).numpy()
    i = np.arange(n)[:, None]
    j = np.arange(n)[None, :]
    p = np.full(n, -1)
    p[:R] = pos
    selfpos = ((j == i) | (j == p[:, None])) & (i < R) & (j < R)
    special = selfpos | (i >= R) | (j >= R)
    return special, selfpos


@pytest.mark.parametrize("R", ROWS)
def test_partner_and_is_negative(ext, R):
    n, nh = _rpad(R), R // 2
    pos = R_.positive_index(R).tolist()
    assert [ext.pair_partner(i, nh) for i in range(R)] == pos
    special, _ = _brute(R, n)
    got = ext.pair_negative_matrix(R, nh, n).numpy()
    assert got.shape == (n, n) and np.array_equal(got, ~special)
    # every valid row has R - 2 negatives
    assert (got[:R].sum(1) == R - 2).all() and not got[R:].any()


@pytest.mark.parametrize("R", ROWS)
def test_tile_drop_every_origin(ext, R):
    """TileMask::drop through every 256-tile origin of the padded square; with diag = false only
    the padding is dropped."""
    n, nh = _rpad(R), R // 2
    special, selfpos = _brute(R, n)
    assert np.array_equal(ext.pair_drop_matrix(R, nh, n, TILE, True).numpy(), special)
    assert np.array_equal(ext.pair_drop_matrix(R, nh, n, TILE, False).numpy(), special & ~selfpos)
    # the rule does not depend on the tiling: 64-element tiles (the 64-column epilogue's origin)
    assert np.array_equal(ext.pair_drop_matrix(R, nh, n, 64, True).numpy(), special)


@pytest.mark.parametrize("R", ROWS)
def test_window_plain(ext, R):
    """Every 64 x 64 and 128 x 64 window, the own block first, second and third of a three-block
    column range: true only where brute force finds no self, positive or padding element."""
    n, nh = _rpad(R), R // 2
    special, _ = _brute(R, n)
    pad_only = (np.arange(n)[:, None] >= R) | (np.arange(n)[None, :] >= R)
    for own in range(3):
        own0 = own * n
        # rows: the own block; columns: three blocks, the own one carrying self and positives
        full = np.concatenate([special if b == own else pad_only for b in range(3)], axis=1)
        n_true = 0
        for nr in (64, 128):
            blocks = full.reshape(n // nr, nr, 3 * n // 64, 64).any(axis=(1, 3))
            for a in range(n // nr):
                for c in range(3 * n // 64):
                    got = ext.pair_window_plain(a * nr, nr, c * 64, 64, own0, R, nh, (c * 64) % n)
                    assert not (got and blocks[a, c]), (R, own0, nr, a, c)
                    n_true += got
        if R >= 600:
            assert n_true > 0, (R, own0)


@pytest.mark.parametrize("R", ROWS)
def test_tile_and_fragment_near(ext, R):
    """False means: no self or positive element in the 256-tile / in the 16 x 16 fragment at block
    offset cb - rb (every tile origin, every fragment)."""
    n, nh = _rpad(R), R // 2
    _, selfpos = _brute(R, n)
    tiles = selfpos.reshape(n // TILE, TILE, n // TILE, TILE).any(axis=(1, 3))
    frags = selfpos.reshape(n // 16, 16, n // 16, 16).any(axis=(1, 3))
    n_far = 0
    for a in range(n // TILE):
        for b in range(n // TILE):
            near = ext.pair_tile_near(R, nh, a * TILE, b * TILE)
            assert near or not tiles[a, b], (R, a, b)
            for fr in range(16):
                for fc in range(16):
                    fn = ext.pair_fragment_near(R, nh, a * TILE, b * TILE, 16 * (fc - fr))
                    assert fn or not frags[16 * a + fr, 16 * b + fc], (R, a, b, fr, fc)
                    n_far += not fn
    assert n_far > 0  # some fragment is cleared: the pre-test is not constantly true
    if R == 1000:  # tile (0, 3): the positives of rows 0..255 are columns 500..755, left of column 768
        assert not ext.pair_tile_near(R, nh, 0, 3 * TILE) and not tiles[0, 3]
