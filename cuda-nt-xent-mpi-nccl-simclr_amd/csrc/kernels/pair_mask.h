// The NT-Xent pair rule, once, for host and device.
//
// Rows 0 .. R-1 of a rank's block are the two views of n_half = R / 2 samples: the partner
// (positive) of row i is p(i) = i +- n_half. Element (i, j) of the block's R x R square of
// cosines is a NEGATIVE unless j == i (self), j == p(i) (positive), or i or j lies in the
// padding (>= R; buffers are padded to Rpad rows). Every kernel that masks, counts or weighs
// pairs takes the rule from here; tests/test_pair_mask_cpu.py checks this header exhaustively on
// the CPU through the _C.pair_* bindings (the same inline functions the kernels compile).
//
// No HIP dependency: under a plain host compiler the functions are ordinary inline functions.
#pragma once

#if defined(__HIP__)
#define NTXENT_PAIR_FN __host__ __device__ __attribute__((always_inline)) inline
#else
#define NTXENT_PAIR_FN inline
#endif

namespace ntxent {
namespace pair {

// p(i): the other view of row i's sample (own-block local index, i < R = 2 n_half).
// The expression itself is a macro for the one site whose code generation depends on seeing it in
// place (dz8_finish: nested in another conditional, the inlined function compiles to different
// branches in the fp8 dZ GEMM); everything else calls partner().
#define NTXENT_PAIR_PARTNER(i, n_half) ((i) < (n_half) ? (i) + (n_half) : (i) - (n_half))
NTXENT_PAIR_FN int partner(int i, int n_half) { return NTXENT_PAIR_PARTNER(i, n_half); }

// The rule in own-block local indices: (i, j) is masked (no negative) when it is the self pair,
// the positive pair or touches the padding.
NTXENT_PAIR_FN bool is_masked(int i, int j, int R, int n_half) {
  return (i >= R) | (j >= R) | (j == i) | (j == partner(i, n_half));
}
NTXENT_PAIR_FN bool is_negative(int i, int j, int R, int n_half) { return !is_masked(i, j, R, n_half); }

// The rule inside one tile of the own block whose element (0, 0) is (row r0, local column c0).
// Element (tile row tr, tile column tc) is the self pair when tc - tr == r0 - c0 (= D0) and the
// positive when tc - tr == D0 + n_half (rows of the first view) or D0 - n_half (second view).
struct TileMask {
  int R, n_half, r0, c0, D0, D1, D2;
  NTXENT_PAIR_FN TileMask(int R_, int n_half_, int r0_, int c0_)
      : R(R_), n_half(n_half_), r0(r0_), c0(c0_), D0(r0_ - c0_), D1(D0 + n_half_), D2(D0 - n_half_) {}

  // True when (tr, tc) is no negative. diag = false leaves the self / positive tests out: for
  // tiles of another rank's block, or when near() below is false.
  NTXENT_PAIR_FN bool drop(int tr, int tc, bool diag = true) const {
    const int gi = r0 + tr, d = tc - tr;
    return (gi >= R) | (c0 + tc >= R) | (diag & ((d == D0) | ((d == D1) & (gi < n_half)) | ((d == D2) & (gi >= n_half))));
  }

  // Conservative pre-tests of the forward GEMM epilogue (wave-uniform there, so only the few
  // fragments that need it run per-lane selects). Contract, both: FALSE means that no self or
  // positive element lies in the tile / fragment; true promises nothing.
  //
  // near(): for a 256 x 256 tile cut into 16 x 16 fragments at block offsets cb - rb in
  // [-240, 240], an element's tc - tr lies within 15 of its fragment's offset, so only a tile with
  // some |D| <= 255 can hold a self or positive element (the diagonal band and the two positive
  // bands of the own block).
  NTXENT_PAIR_FN bool near() const {
    return (D0 <= 255 && D0 >= -255) || (D1 <= 255 && D1 >= -255) || (D2 <= 255 && D2 >= -255);
  }
  // fragment_near(off): the 16 x 16 fragment at block offset off = cb - rb holds tc - tr in
  // [off - 15, off + 15].
  NTXENT_PAIR_FN bool fragment_near(int off) const {
    return (off - D0 <= 15 && D0 - off <= 15) || (off - D1 <= 15 && D1 - off <= 15) || (off - D2 <= 15 && D2 - off <= 15);
  }
};

// Conservative "plain window" test of the coefficient epilogues. The window is rows
// [r_lo, r_lo + nr) of the own block (local indices) by columns [c_lo, c_lo + nc) of the gathered
// column range (global indices: the own block starts at column own0, block b at b * Rpad);
// c_local is the block-local index of column c_lo (the window lies in one block). Contract: TRUE
// means that no self, positive or padding element lies in the window; false promises nothing.
// (The selfs of the rows are the columns own0 + [r_lo, r_lo + nr), the positives lie in that
// range shifted by +n_half or -n_half: the window is plain if its columns miss all three.)
NTXENT_PAIR_FN bool window_plain(int r_lo, int nr, int c_lo, int nc, int own0, int R, int n_half, int c_local) {
  const int c_hi = c_lo + nc;
  auto hits = [&](int a0) { return a0 < c_hi && c_lo < a0 + nr; };
  return r_lo + nr <= R && c_local + nc <= R && !hits(own0 + r_lo) && !hits(own0 + r_lo + n_half) &&
         !hits(own0 + r_lo - n_half);
}

}  // namespace pair
}  // namespace ntxent
