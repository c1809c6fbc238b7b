// Cross-view InfoNCE kernels for gfx950: the CLIP-form two-tower loss, rank r of W ranks.
//
// Every rank holds n pairs, stacked as everywhere else ([view 1 (n); view 2 (n); zero pad] =
// launch_prep's unit rows, rows_pad of them); zq holds the W ranks' rows slot by slot and the global
// batch in pair order is [a_0; ..; a_{W-1}; b_0; ..; b_{W-1}] (N = W n pairs). A row's columns are the
// rows of the OTHER view only, the positive included:
//   lse_i = log sum_{j : view(j) != view(i)} exp(cos_ij / tau),  loss = 1/2N sum_i (lse_i - cos_ip / tau)
// Per side v the rows are view v of this rank and the columns view 1 - v of every slot; column tile J
// of a side's n x N block is local tile J % nT of slot J / nT (nT = n_pad / 128), and the positive of
// local row l is column l of the own slot. With P_ij = exp(cos_ij / tau - lse_i) the gradient block
// of a side is G_ij = P_ij + P_ji - 2 [j = p(i)], and (C z)[side rows] = G Z(other view).
//
//   xview_fwd_kernel  : one 128 x 128 tile (side, I, slot q, local tile Jl) per workgroup by
//                       tile128.h's MFMA loop. Epilogue: negatives-only (max, sum exp2) per row,
//                       reduced in the wave and across the two waves in a fixed order, and stored in
//                       launch_lse's `part` layout, slot q * nT + Jl, row side * n + l. Every (slot,
//                       valid row) is written exactly once, so any split of the slots over launches
//                       (own slot first, while the others are gathered) gives the same bits; side 0's
//                       own diagonal tiles also store the pairs' positive logits (ypos), so a pair's
//                       positive and its negatives come from the same MFMA arithmetic.
//   xview_lse_kernel  : a thread per positive pair merges the W * nT slots of both rows in slot order
//                       with the positive logit (negatives-only LSE merged with y_pos and the positive
//                       coefficient -(sigmoid(lse_neg_i - y) + sigmoid(lse_neg_p - y)), as launch_lse:
//                       stable when P_ip -> 1) into this rank's slot of lse2; the loss terms are
//                       formed in fp64 relative to y_pos.
//   xview_loss_kernel : their sum in a fixed order (one block, fp64 tree). No atomics anywhere.
//   xview_side_coef_kernel : the same tile GEMM again for ONE side; the epilogue forms the tile of G
//                       from the gathered lse2 and cpos and stores it once, row-major [n_pad][W n_pad]
//                       planes in the compute dtype (zeros outside the valid rows and columns): one
//                       fp32 plane, or for 16-bit plans G rounded to the dtype and the scaled residual
//                       of that rounding, so that the MFMA operands carry the coefficients to about
//                       twice the dtype's mantissa (a gradient of equal coefficients is otherwise off
//                       by the dtype's rounding of that one number). The only n N data, 4 n_pad W n_pad
//                       bytes in every plan. Side 1 swaps the operand roles and so gives the rows of
//                       G^T directly.
//   xview_transpose_kernel : Zt[v][e][q n_pad + c] = zq[q rows_pad + v n + c][e] for every slot q,
//                       both views aligned at column 0 of their slot and zero padded to n_pad columns
//                       and roundup(dim_k, 128) rows (view 2 starts at row n, usually not tile aligned).
//   xview_dz_kernel   : a side's rows of out = G Z: one 128 x 128 output tile per workgroup, K =
//                       W n_pad per plane (slots ascending inside a plane), both operands streamed
//                       K-major by LDS-DMA in the same MFMA loop (tile128.h's, over the K-steps of
//                       every plane); 16-bit plans run the residual plane, scale the accumulators back
//                       and run the hi plane. fp32 output slab. Each output element is one workgroup's
//                       fixed-order sum: deterministic.
// launch_norm_bwd (with dot_out) and launch_tau_grad finish the backward as they are.
//
// One GPU is W = 1, r = 0 of the same kernels, except in two places where one block S12 = Z1 Z2^T
// serves both sides:
//   - the forward runs side 0's nT x nT tiles only, with kCols: the tile's columns are the view-2
//     rows' logits, so the epilogue also reduces (max, sum exp2) per column and stores them as the
//     view-2 rows' partials, slot I (half the forward FLOPs of two sides);
//   - the backward stores G once (side 0) and xview_gt_kernel transposes the planes in place between
//     the two dZ products, instead of a second coefficient pass.
//
// The pairwise sigmoid loss (the SigLIP form) is two more epilogues of the same tile GEMM,
// xview_sigmoid_fwd_kernel and xview_sigmoid_coef_kernel (below, beside the family): no LSE, no
// column partials; its coefficient block goes through the same transposes and dZ products. 16-bit
// plans take the positives' cosines from the fp32 unit rows (xview_sigmoid_pos_kernel). Rank r of W:
// the forward runs side 0's n x W n block alone (every global pair is computed once, on the rank
// that holds its row a_i), the coefficient pass one side at a time as xview_side_coef_kernel; one
// GPU is W = 1, side 0 of both, with the in-place transpose in place of side 1.
// The block form of both epilogues (kBlock) and of the dZ product (kAccum) serves the ring exchange:
// this rank's one slot against one other rank's slot at a time, the same arithmetic, the partials at
// the gather launches' places and the dZ slab accumulated block after block (the rows_q / kslots = 1
// forms of launch_xview_sigmoid_dist_* and launch_xview_dist_zt / _dz).
#include "../include/ntxent/ntxent.h"
#include "device_common.h"
#include "host_common.h"
#include "tile128.h"

namespace ntxent {
namespace dev {

constexpr int kXvTile = kTile128;
constexpr int kXvThreads = kTile128Threads;

// zq holds W slots of rows_pad rows. With n + n_pad <= rows_pad no 128-row stage leaves its slot.
struct XvParams {
  const char* zq;     // [world * rows_pad][ldb bytes] unit rows (zero K padding, zero pad rows)
  long long ldb;      // row stride in bytes
  int n;              // pairs per rank
  int rows_pad;
  int nk;             // 128-byte K-steps per row of zq
  int nT;             // n_pad / 128: 128-row tiles per view of a slot
  int world, rank;
  int q_lo, nq, q_skip;  // forward: the launch's column slots, nq of them from q_lo on, q_skip left out
  int side;           // coefficient pass: the side
  float scale2;       // log2(e) / tau: cosine -> logit in log2 units
  float2* part;       // forward: [world * nT][rows_pad] (launch_lse's layout), row side * n + l
  float* ypos;        // forward: [>= n] positive logits of the pairs (log2 units), written
  const float* lse2;  // coefficient pass: [world * rows_pad] gathered LSE (log2 units, positive included)
  const float* cpos;  //                   [rows_pad] positive coefficients of this rank's rows
  char* gbuf;         // [planes][n_pad][ldg bytes] G in the compute dtype (16-bit: residual plane, hi plane)
  long long ldg;
  long long plane_bytes;
  // block form (kBlock kernels): zq is this rank's own ONE slot [rows_pad][ldb], zcol a one-slot buffer
  // of the same shape that holds rank q_lo's rows (the own block: zq itself). q_lo is the slot's
  // identity: it drives own = (q == rank), the positive test and the output place, no buffer index.
  const char* zcol;
};
// 16-bit plans: the residual plane holds (G - hi) * kXvLoScale, clear of fp16's subnormals; the dZ
// runs it first and scales its accumulators back (a power of two: exact) before the hi plane.
constexpr float kXvLoScale = 2048.f;

// acc = tile (I, Jl of slot q) of side `side`: rows side * n + I * 128 .. of the own slot against
// rows (1 - side) * n + Jl * 128 .. of slot q. Ends with a block barrier: the caller's epilogue may
// reuse the staging images. kBlock: the rows from the one-slot p.zq, the columns from the one-slot
// p.zcol (rank q's rows); q does not index a buffer.
template <typename T, bool kBlock = false>
__device__ __forceinline__ void xv_tile_gemm(const XvParams& p, int side, int I, int q, int Jl, lds_char* lds,
                                             f32x4 (&acc)[4][4]) {
  const long long aslot = kBlock ? 0 : (long long)p.rank * p.rows_pad, bslot = kBlock ? 0 : (long long)q * p.rows_pad;
  const char* arow = p.zq + (aslot + (long long)side * p.n + (long long)I * kXvTile) * p.ldb;
  const char* brow = (kBlock ? p.zcol : p.zq) + (bslot + (long long)(1 - side) * p.n + (long long)Jl * kXvTile) * p.ldb;
  tile128_gemm<T>(
      lds, p.nk, [&](int k) { return Tile128Src{arow + (long long)k * kKStepBytes, p.ldb}; },
      [&](int k) { return Tile128Src{brow + (long long)k * kKStepBytes, p.ldb}; }, false, Tile128Plain{}, acc);
}

// ---- forward: LSE partials of the tile's rows, slot q * nT + Jl -------------------------------------
// kCols (one GPU: world 1, side 0's tiles): also of its columns, the other view's rows, slot I.
// Without it the other view's rows get theirs from the other side's tiles.
template <typename T, bool kCols>
__global__ __launch_bounds__(kXvThreads) void xview_fwd_kernel(const XvParams p) {
  // ONE __shared__ object (staging ring, reused by the epilogue)
  __shared__ __attribute__((aligned(16))) char smem[kTile128Lds];
  lds_char* lds = (lds_char*)smem;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, r16 = lane & 15, g = lane >> 4;
  const int b = xcd_remap(blockIdx.x, gridDim.x);
  const int ncol = p.nq * p.nT, per_side = p.nT * ncol;
  const int side = b / per_side, rem = b - side * per_side;
  const int I = rem / ncol, jj = rem - I * ncol;
  int q = p.q_lo + jj / p.nT;
  const int Jl = jj % p.nT;
  if (p.q_skip >= 0 && q >= p.q_skip) ++q;
  const int n = p.n;
  const bool own = q == p.rank;

  f32x4 acc[4][4];
  xv_tile_gemm<T>(p, side, I, q, Jl, lds, acc);

  // epilogue LDS: per-wave-column row (max, sum) | kCols: per-wave-row column (max, sum)
  float* s_rm = reinterpret_cast<float*>(smem);  // [2][128]
  float* s_rs = s_rm + 2 * kXvTile;
  float* s_cm = s_rs + 2 * kXvTile;
  float* s_cs = s_cm + 2 * kXvTile;

  int cl[4];
  [[maybe_unused]] float cm[4], cs[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    cl[ni] = Jl * kXvTile + 64 * wc + 16 * ni + r16;
    if constexpr (kCols) {
      cm[ni] = kNegInf;
      cs[ni] = 0.f;
    }
  }
  // pass 1: logits (log2 units; -inf for what is no negative) and the maxima
  float rmx[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int li = I * kXvTile + 64 * wr + 16 * mi + 4 * g + r;
      float m = kNegInf;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        // local rows and columns at or beyond n are the other view's rows or slot padding: masked by
        // index. The positive is the own slot's column of the same local index and nothing else; it
        // joins in xview_lse_kernel.
        const bool in = (li < n) & (cl[ni] < n);
        const bool pos = own & (cl[ni] == li);
        const float yv = acc[mi][ni][r] * p.scale2;
        // the pair's positive logit from the same MFMA sum as its negatives (one lane of one tile
        // per pair): rows whose cosines are equal then have exactly equal logits
        if (in & pos & (side == 0)) p.ypos[li] = yv;
        const float y = (in & !pos) ? yv : kNegInf;
        acc[mi][ni][r] = y;
        m = fmaxf(m, y);
        if constexpr (kCols) cm[ni] = fmaxf(cm[ni], y);
      }
      rmx[mi][r] = row16_max(m);
    }
  if constexpr (kCols) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) cm[ni] = xrow_max(cm[ni]);
  }
  // pass 2: sums of exp2 against the maxima
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rt = 64 * wr + 16 * mi + 4 * g + r;
      const float mr = rmx[mi][r];
      float s = 0.f;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const float y = acc[mi][ni][r];
        const bool ok = y != kNegInf;
        s += ok ? fast_exp2(y - mr) : 0.f;
        if constexpr (kCols) cs[ni] += ok ? fast_exp2(y - cm[ni]) : 0.f;
      }
      s = row16_sum(s);
      if (r16 == 0) {
        s_rm[wc * kXvTile + rt] = mr;
        s_rs[wc * kXvTile + rt] = s;
      }
    }
  if constexpr (kCols) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      cs[ni] = xrow_sum(cs[ni]);
      if (g == 0) {
        const int ct = 64 * wc + 16 * ni + r16;
        s_cm[wr * kXvTile + ct] = cm[ni];
        s_cs[wr * kXvTile + ct] = cs[ni];
      }
    }
  }
  __syncthreads();
  // threads [0, 128): the tile's rows -> slot q * nT + Jl; kCols, [128, 256): its columns -> slot I
  const bool col = kCols && tid >= kXvTile;
  if (kCols || tid < kXvTile) {
    const int t = tid & (kXvTile - 1);
    const float* sm = col ? s_cm : s_rm;
    const float* ss = col ? s_cs : s_rs;
    float m = sm[t], s = ss[t];
    lse_merge(m, s, sm[kXvTile + t], ss[kXvTile + t]);
    const int idx = (col ? Jl : I) * kXvTile + t;  // index within the view
    if (idx < n) {
      const long long slot = col ? I : (long long)q * p.nT + Jl;
      p.part[slot * p.rows_pad + (col ? 1 - side : side) * n + idx] = make_float2(m, s);
    }
  }
}

// ---- forward: merge of the partials, row statistics and the loss ---------------------------------
// Row statistics from a row's merged negatives-only (max, sum) state and the pair's positive logit
// (all log2 units): returns lse2 = logaddexp2(lse_neg, y_pos) and a = 1 - P_ip = sigmoid(lse_neg -
// y_pos) as device_common.h's finish_row does; the loss term softplus(lse_neg - y_pos) is formed in
// fp64 from (m - y_pos) + log2 s, the difference taken before the logarithm is added: both logits
// are of size 1 / tau and their fp32 sum m + log2 s would round at that size, not at the loss's.
__device__ __forceinline__ float xv_finish_row(float m, float s, float yp, double& loss, float& a) {
  const bool empty = m == kNegInf || s <= 0.f;
  const float neg2 = empty ? kNegInf : m + log2f(s);
  const float mx = fmaxf(neg2, yp);
  const float l2 = mx + log2f(exp2f(neg2 - mx) + exp2f(yp - mx));
  const double x = empty ? -(double)kPosInf : (((double)m - (double)yp) + log2((double)s)) * 0.6931471805599453;
  loss = x > 0.0 ? x + log1p(exp(-x)) : log1p(exp(x));
  a = (float)(1.0 / (1.0 + exp(-x)));
  return l2;
}

// One thread per positive pair (i, i + N): the nT slots of both rows merged in slot order, then
// lse2 / cpos of both rows and the pair's loss terms (lpair, fp64). The threads behind the pairs
// zero the pad rows [R, rows_pad) of lse2 / cpos.
__global__ __launch_bounds__(256) void xview_lse_kernel(const float2* __restrict__ part, const float* __restrict__ ypos,
                                                        float* __restrict__ lse2, float* __restrict__ cpos,
                                                        double* __restrict__ lpair, int N, int rows_pad, int nT) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) {
    float mi = kNegInf, si = 0.f, mj = kNegInf, sj = 0.f;
    for (int t = 0; t < nT; ++t) {
      const float2 a = part[(long long)t * rows_pad + i], b = part[(long long)t * rows_pad + N + i];
      lse_merge(mi, si, a.x, a.y);
      lse_merge(mj, sj, b.x, b.y);
    }
    const float yp = ypos[i];
    double li, lj;
    float ai, aj;
    lse2[i] = xv_finish_row(mi, si, yp, li, ai);
    lse2[N + i] = xv_finish_row(mj, sj, yp, lj, aj);
    // C_ip = P_ip + P_pi - 2 = -(a_i + a_p): no 1 - P cancellation when P_ip -> 1
    cpos[i] = -(ai + aj);
    cpos[N + i] = -(ai + aj);
    lpair[i] = li + lj;
  } else if (i - N < rows_pad - 2 * N) {
    lse2[2 * N + (i - N)] = 0.f;
    cpos[2 * N + (i - N)] = 0.f;
  }
}

// (sum of lpair) / denom. One GPU: denom = R and the loss goes to loss[0]. Distributed: denom = the
// global row count and the rank's share stays in fp64 (share64[0], loss null): the shares are summed
// across ranks before the one rounding to fp32. One block: thread t sums pairs t, t + 1024, ... in
// order, then a fixed halving tree (fp64): deterministic, no atomics.
constexpr int kXvSumThreads = 1024;
__global__ __launch_bounds__(kXvSumThreads) void xview_loss_kernel(const double* __restrict__ lpair, int N,
                                                                   double denom, float* __restrict__ loss,
                                                                   double* __restrict__ share64) {
  __shared__ double red[kXvSumThreads];
  double t = 0.0;
  for (int i = threadIdx.x; i < N; i += kXvSumThreads) t += lpair[i];
  red[threadIdx.x] = t;
  __syncthreads();
#pragma unroll
  for (int n = kXvSumThreads / 2; n > 0; n >>= 1) {
    if ((int)threadIdx.x < n) red[threadIdx.x] += red[threadIdx.x + n];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (loss) loss[0] = (float)(red[0] / denom);
    else share64[0] = red[0] / denom;
  }
}

// ---- backward: tile (I, J) of one side's n_pad x W n_pad block G, stored once ----------------------
template <typename T>
__global__ __launch_bounds__(kXvThreads) void xview_side_coef_kernel(const XvParams p) {
  __shared__ __attribute__((aligned(16))) char smem[kTile128Lds];
  lds_char* lds = (lds_char*)smem;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, r16 = lane & 15, g = lane >> 4;
  const int b = xcd_remap(blockIdx.x, gridDim.x);
  const int ncol = p.world * p.nT;
  const int I = b / ncol, J = b - I * ncol;
  const int q = J / p.nT, Jl = J - q * p.nT;
  const int n = p.n, side = p.side;
  const bool own = q == p.rank;

  f32x4 acc[4][4];
  xv_tile_gemm<T>(p, side, I, q, Jl, lds, acc);

  // the tile's planes in the compute dtype, row-major [128][128] each, over the staging images
  // (64 KiB): fp32 plans one plane, G; 16-bit plans the residual plane (G - hi) * 2^11, then hi =
  // G rounded to T. The dZ adds both, so the coefficients carry about 2 x the operand's mantissa.
  constexpr bool kSplit = sizeof(T) == 2;
  constexpr int kPlaneElems = kXvTile * kXvTile;
  T* s_g = reinterpret_cast<T*>(smem);
  const float* lrow = p.lse2 + (long long)p.rank * p.rows_pad + side * n;
  const float* lcol = p.lse2 + (long long)q * p.rows_pad + (1 - side) * n;
  int cl[4];
  float lc[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    cl[ni] = Jl * kXvTile + 64 * wc + 16 * ni + r16;
    lc[ni] = cl[ni] < n ? lcol[cl[ni]] : 0.f;
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rt = 64 * wr + 16 * mi + 4 * g + r;
      const int li = I * kXvTile + rt;
      const float lr = li < n ? lrow[li] : 0.f;
      const float cp = li < n ? p.cpos[side * n + li] : 0.f;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const float y = acc[mi][ni][r] * p.scale2;
        const bool ok = (li < n) & (cl[ni] < n);
        const float c = fast_exp2(y - lr) + fast_exp2(y - lc[ni]);
        // selects, not products: outside the valid rows and columns the exponentials may overflow
        const float v = ok ? ((own & (cl[ni] == li)) ? cp : c) : 0.f;
        const int at = rt * kXvTile + 64 * wc + 16 * ni + r16;
        const T hi = from_f32<T>(v);
        if constexpr (kSplit) {
          s_g[at] = from_f32<T>((v - to_f32<T>(hi)) * kXvLoScale);
          s_g[kPlaneElems + at] = hi;
        } else {
          s_g[at] = hi;
        }
      }
    }
  __syncthreads();
  // 16-byte chunks, rows contiguous: 8 * sizeof(T) chunks per row, 4096 chunks in all
  constexpr int kCpr = kXvTile * (int)sizeof(T) / 16;
  constexpr int kCpp = kCpr * kXvTile;  // chunks per plane
  char* gt = p.gbuf + (long long)I * kXvTile * p.ldg + (long long)J * kXvTile * (int)sizeof(T);
#pragma unroll
  for (int c = 0; c < kTile128Lds / 16 / kXvThreads; ++c) {
    const int idx = c * kXvThreads + tid;
    const int plane = idx / kCpp, in = idx - plane * kCpp;
    const int row = in / kCpr, cc = in - row * kCpr;
    const u32x4 v = *reinterpret_cast<const u32x4*>(smem + idx * 16);
    *reinterpret_cast<u32x4*>(gt + plane * p.plane_bytes + (long long)row * p.ldg + cc * 16) = v;
  }
}

// ---- Zt[v][e][q slot_cols + c] = zq[q slot_rows + v N + c][e] (blockIdx.z = 2 q + v) ---------------
template <typename T>
__global__ __launch_bounds__(256) void xview_transpose_kernel(const T* __restrict__ zq, T* __restrict__ zt, int N,
                                                              int dim_k, long long ldk, int En, long long ldz,
                                                              long long slot_rows, long long slot_cols) {
  __shared__ T tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c0 = blockIdx.x * 64, e0 = blockIdx.y * 64, v = blockIdx.z & 1;
  zq += (long long)(blockIdx.z >> 1) * slot_rows * ldk;
  zt += (long long)(blockIdx.z >> 1) * slot_cols;
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int c = c0 + ty + 4 * j, e = e0 + tx;
    tile[ty + 4 * j][tx] = (c < N && e < dim_k) ? zq[((long long)v * N + c) * ldk + e] : from_f32<T>(0.f);
  }
  __syncthreads();
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int e = e0 + ty + 4 * j, c = c0 + tx;
    zt[((long long)v * En + e) * ldz + c] = tile[tx][ty + 4 * j];
  }
}

// ---- G -> G^T in place (every plane) -------------------------------------------------------------
// One workgroup per pair of 64 x 64 tiles (bx <= by) of a square [np][np] plane: both tiles go
// through LDS and come back transposed in each other's place (a diagonal tile in its own). No
// element is touched by two workgroups.
template <typename T>
__global__ __launch_bounds__(256) void xview_gt_kernel(T* __restrict__ gbuf, long long np, long long plane_elems) {
  const int bx = blockIdx.x, by = blockIdx.y;
  if (bx > by) return;
  __shared__ T ta[64][65], tb[64][65];
  T* gp = gbuf + (long long)blockIdx.z * plane_elems;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  T* a = gp + ((long long)by * 64) * np + (long long)bx * 64;  // tile (by, bx)
  T* b = gp + ((long long)bx * 64) * np + (long long)by * 64;  // tile (bx, by)
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int r = ty + 4 * j;
    ta[r][tx] = a[r * np + tx];
    tb[r][tx] = b[r * np + tx];
  }
  __syncthreads();
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int r = ty + 4 * j;
    a[r * np + tx] = tb[tx][r];
    if (bx != by) b[r * np + tx] = ta[tx][r];
  }
}

// ---- out = A Z^T-rows: G Z2 (side 0, A = G) | G^T Z1 (side 1, A = G^T) ----------------------------
struct XvDzParams {
  const char* gbuf;  // [planes][n_pad][ldg bytes]: the side's G (one GPU, side 1: G^T after xview_gt_kernel)
  long long ldg;
  long long plane_bytes;
  int planes;        // 1, or 2: the residual plane (scaled by kXvLoScale), then the hi plane
  const char* zt;    // [2][En][ldz bytes]
  long long ldz;
  int En;            // roundup(dim_k, 128)
  int n_half;
  int side;          // the view whose rows are written; B is the other view's Zt
  int nk;            // 128-byte K-steps over W n_pad (per plane)
  float* out;        // [rows_pad][ldo]
  long long ldo;
};

// kAccum (the ring's later blocks): out[m][e] = out[m][e] + acc with plain loads and stores. One
// workgroup owns each element per launch and the launches are stream-ordered: a fixed order, no atomics.
template <typename T, bool kAccum = false>
__global__ __launch_bounds__(kXvThreads) void xview_dz_kernel(const XvDzParams p) {
  __shared__ __attribute__((aligned(16))) char smem[kTile128Lds];
  lds_char* lds = (lds_char*)smem;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, r16 = lane & 15, g = lane >> 4;
  const int Ei = blockIdx.x, Mi = blockIdx.y, side = p.side;

  // A: rows Mi * 128 .. of the coefficient planes; B: rows e of the OTHER view's Zt; K along both
  const char* arow = p.gbuf + (long long)Mi * kXvTile * p.ldg;
  const char* brow = p.zt + ((long long)(1 - side) * p.En + (long long)Ei * kXvTile) * p.ldz;

  // steps kk = plane * nk + k: the planes one after the other over the same B K-steps. No end
  // barrier: the epilogue does not touch LDS.
  const int nk = p.nk;
  f32x4 acc[4][4];
  tile128_gemm<T, /*kEndBarrier=*/false>(
      lds, p.planes * nk,
      [&](int kk) {
        const int pl = kk >= nk ? 1 : 0, k = kk - pl * nk;
        return Tile128Src{arow + (long long)pl * p.plane_bytes + (long long)k * kKStepBytes, p.ldg};
      },
      [&](int kk) { return Tile128Src{brow + (long long)(kk >= nk ? kk - nk : kk) * kKStepBytes, p.ldz}; }, false,
      [&](int kk, f32x4(&c)[4][4]) {
        if (kk == nk) {  // the residual plane is done: back to G's scale before the hi plane
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) c[mi][ni] *= 1.0f / kXvLoScale;
        }
      },
      acc);

  // rows of this view at or beyond N do not exist (the coefficients are zero there anyway)
  float* out = p.out;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = Mi * kXvTile + 64 * wr + 16 * mi + 4 * g + r;
      if (m < p.n_half) {
        float* orow = out + ((long long)side * p.n_half + m) * p.ldo + (long long)Ei * kXvTile + 64 * wc + r16;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          if constexpr (kAccum) orow[16 * ni] = orow[16 * ni] + acc[mi][ni][r];
          else orow[16 * ni] = acc[mi][ni][r];
        }
      }
    }
}

// ---- pairwise sigmoid loss (the SigLIP form) ---------------------------------------------------------
// x_ij = a_i . b_j / tau + bias over the n x W n pairs of this rank's view-1 rows against the view-2
// rows of every slot (side 0's nT x W nT tiles: every global pair is computed once; one GPU is world
// 1, rank 0); the positive of local row i is column i of the own slot:
//   loss = 1/N sum_ij softplus(-s_ij x_ij),  s_ii = +1, s_ij = -1 otherwise,  N = W n.
// With G_ij = sigmoid(x_ij) (i != j) and G_ii = -sigmoid(-x_ii) the coefficient block is C = 2 G: the
// factor (a power of two: exact) makes launch_norm_bwd's grad_out / (R tau) the loss's 1 / (n tau) and
// launch_tau_grad's -(1 / (2 R tau^2)) sum_i dot_i over both views' rows dL/dtau, so the dZ products,
// the normalisation backward and the temperature gradient serve as they are.
struct XvSigParams {
  XvParams x;        // the tile GEMM's operands; the coefficient pass: gbuf / ldg / plane_bytes as well
  // x_ij in log2 units = cos_ij * scale2 + bias2, formed in fp64 and rounded to fp32 once per pair: an
  // fp32 scale and bias would be off by their own rounding in the same direction for every pair, which
  // no sum over the pairs averages out (the bias gradient's sum least of all)
  double scale2;     // log2(e) / tau
  double bias2;      // log2(e) * bias
  double* lpart;    // forward: [nT][world * nT] the tiles' sums of softplus terms, tile (I, q, Jl) at its place
  float* bias_part;  // coefficient pass: [nT * world * nT][4] the waves' sums of C = 2 G; null (side 1): not stored
  // 16-bit plans: [n] the pairs' cosines a_i . b_i from the input rows in fp32
  // (xview_sigmoid_pos_kernel), taken for the diagonal in place of the tile's sum; null: the tile's.
  // The N positives carry the loss, dL/dbias and dL/dtau once bias pushes the negatives down, every
  // x_ii enters with weight 1 / N, and the mean shift of cos_ii from rounding the unit rows to 16 bits
  // (2.6e-5 in bf16) goes through undiminished: no normaliser cancels it as a softmax loss's does.
  const float* pos_cos;
};

// cos[i] = z_i . z_{i + n} of the fp32 unit rows z = h * inv, the operands an fp32 plan has (so rows
// that are exact there, one-hot ones, are exact here): one wave per pair, the products summed in fp64
// in a fixed order (lane, then the wave's lanes).
template <typename Tin>
__global__ __launch_bounds__(256) void xview_sigmoid_pos_kernel(const Tin* __restrict__ h, const float* __restrict__ inv,
                                                                float* __restrict__ cos, int n, int d) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;  // whole wave
  const Tin* a = h + (long long)i * d;
  const Tin* b = h + (long long)(i + n) * d;
  const float ia = inv[i], ib = inv[i + n];
  double s = 0.0;
#pragma unroll 8  // the loads of eight steps in flight; the sum keeps its order
  for (int e = lane; e < d; e += 64) s += (double)(to_f32<Tin>(a[e]) * ia) * (double)(to_f32<Tin>(b[e]) * ib);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
  if (lane == 0) cos[i] = (float)s;
}

// The pairs' cosines of the rows of a diagonal tile this lane holds (pos_cos given), else zeros.
__device__ __forceinline__ void xv_sig_load_pos(const XvSigParams& ps, bool diag, int row0, int g, float (&pc)[4][4]) {
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) pc[mi][r] = 0.f;
  if (diag && ps.pos_cos) {  // block-uniform
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int li = row0 + 16 * mi + 4 * g + r;
        if (li < ps.x.n) pc[mi][r] = ps.pos_cos[li];
      }
  }
}

// Forward: tile (I, Jl)'s sum of softplus terms, natural-log units. softplus(t) = max(t, 0) +
// log1p(e^-|t|): the log1p form keeps a negative's term (e^-20 at cos = -1, tau = 0.1, bias = -10)
// where log(1 + e) would return 0. Rows and columns at or beyond n contribute nothing, selected by
// index (a pad column has cos = 0 and would add softplus(bias)). Fixed order: a lane's 64 terms, the
// wave's 64 lanes, the four waves; fp64 from the lane on, so the loss is rounded to fp32 once, at
// its end. One partial per tile, no atomics.
// kBlock: the nT x nT tiles of a_r (p.zq, one slot) against b_q (p.zcol, one slot), the launch's one
// slot q = q_lo (nq = 1, no q_skip); the tile's partial goes to the same place of lpart as below.
template <typename T, bool kBlock = false>
__global__ __launch_bounds__(kXvThreads) void xview_sigmoid_fwd_kernel(const XvSigParams ps) {
  __shared__ __attribute__((aligned(16))) char smem[kTile128Lds];
  lds_char* lds = (lds_char*)smem;
  const XvParams& p = ps.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, r16 = lane & 15, g = lane >> 4;
  const int b = xcd_remap(blockIdx.x, gridDim.x);
  // side 0's tiles (I, slot q, Jl) of the launch's slots, as xview_fwd_kernel walks a side's
  const int ncol = p.nq * p.nT;
  const int I = b / ncol, jj = b - I * ncol;
  int q = p.q_lo + jj / p.nT;
  const int Jl = jj % p.nT;
  if (p.q_skip >= 0 && q >= p.q_skip) ++q;
  const int n = p.n;
  const bool own = q == p.rank;

  f32x4 acc[4][4];
  xv_tile_gemm<T, kBlock>(p, 0, I, q, Jl, lds, acc);

  int cl[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) cl[ni] = Jl * kXvTile + 64 * wc + 16 * ni + r16;
  const bool fine_pos = ps.pos_cos != nullptr;
  float pc[4][4];
  xv_sig_load_pos(ps, own && Jl == I, I * kXvTile + 64 * wr, g, pc);
  double sum = 0.0;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int li = I * kXvTile + 64 * wr + 16 * mi + 4 * g + r;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const bool in = (li < n) & (cl[ni] < n);
        const bool pos = own & (cl[ni] == li);  // only in a diagonal tile (Jl == I) of the own slot
        const double x2 = fma((double)((pos & fine_pos) ? pc[mi][r] : acc[mi][ni][r]), ps.scale2, ps.bias2);
        const double t2 = pos ? -x2 : x2;  // -s_ij x_ij
        const double sp = fmax(t2, 0.0) * 0.6931471805599453 + (double)log1pf(fast_exp2(-fabsf((float)t2)));
        sum += in ? sp : 0.0;
      }
    }
  // the wave's lanes, then the four waves (the staging images are free: xv_tile_gemm ended with a barrier)
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) sum += __shfl_xor(sum, m, 64);
  double* s_w = reinterpret_cast<double*>(smem);
  if (lane == 0) s_w[w] = sum;
  __syncthreads();
  // the tile's own place, whichever launch runs it: the sum's order does not depend on the split
  if (tid == 0) ps.lpart[((long long)I * p.world + q) * p.nT + Jl] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// Coefficient pass: tile (I, J) of side p.side's n_pad x W n_pad block (side 1: rows b_r against a of
// every slot; x is symmetric in that swap, so these are the rows of C^T), stored as
// xview_side_coef_kernel stores G (one fp32 plane, or the
// residual plane scaled by kXvLoScale and the hi plane; exact zeros outside the valid rows and
// columns), with C = 2 G: 2 sigmoid(x) = 2 / (1 + e^-x) off the diagonal and, formed directly,
// -2 sigmoid(-x) = -2 / (1 + e^x) on it (an overflowing exponential gives the exact limit 0). The bias
// gradient's partials are taken from the fp32 values before they are rounded to the planes: the plane
// image fills the whole __shared__ object, so every wave reduces in its registers and stores one
// fp32 partial to bias_part[tile][wave].
// kBlock: one side of the ONE block of slot q = q_lo, nT x nT tiles of the one-slot operands, stored as
// planes [n_pad][n_pad] (J = Jl); the bias partials go to the tile's place in the n_pad x W n_pad
// block, ((I W + q) nT + Jl) * 4 + wave, which is what b * 4 + w is below.
template <typename T, bool kBlock = false>
__global__ __launch_bounds__(kXvThreads) void xview_sigmoid_coef_kernel(const XvSigParams ps) {
  __shared__ __attribute__((aligned(16))) char smem[kTile128Lds];
  lds_char* lds = (lds_char*)smem;
  const XvParams& p = ps.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, r16 = lane & 15, g = lane >> 4;
  const int b = xcd_remap(blockIdx.x, gridDim.x);
  // tile (I, J) of one side's n_pad x W n_pad block, as xview_side_coef_kernel
  const int ncol = kBlock ? p.nT : p.world * p.nT;
  const int I = b / ncol, J = b - I * ncol;
  const int q = kBlock ? p.q_lo : J / p.nT, Jl = kBlock ? J : J - q * p.nT;
  const int n = p.n;
  const bool own = q == p.rank;
  const int bplace = kBlock ? (I * p.world + q) * p.nT + Jl : b;

  f32x4 acc[4][4];
  xv_tile_gemm<T, kBlock>(p, p.side, I, q, Jl, lds, acc);

  constexpr bool kSplit = sizeof(T) == 2;
  constexpr int kPlaneElems = kXvTile * kXvTile;
  T* s_g = reinterpret_cast<T*>(smem);
  int cl[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) cl[ni] = Jl * kXvTile + 64 * wc + 16 * ni + r16;
  const bool fine_pos = ps.pos_cos != nullptr;
  float pc[4][4];
  xv_sig_load_pos(ps, own && Jl == I, I * kXvTile + 64 * wr, g, pc);
  float bsum = 0.f;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rt = 64 * wr + 16 * mi + 4 * g + r;
      const int li = I * kXvTile + rt;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const bool ok = (li < n) & (cl[ni] < n);
        const bool pos = own & (cl[ni] == li);
        const float x2 = (float)fma((double)((pos & fine_pos) ? pc[mi][r] : acc[mi][ni][r]), ps.scale2, ps.bias2);
        const float c = (pos ? -2.f : 2.f) / (1.f + fast_exp2(pos ? x2 : -x2));
        // a select, not a product: zeros outside the valid rows and columns
        const float v = ok ? c : 0.f;
        bsum += v;
        const int at = rt * kXvTile + 64 * wc + 16 * ni + r16;
        const T hi = from_f32<T>(v);
        if constexpr (kSplit) {
          s_g[at] = from_f32<T>((v - to_f32<T>(hi)) * kXvLoScale);
          s_g[kPlaneElems + at] = hi;
        } else {
          s_g[at] = hi;
        }
      }
    }
  bsum = wave_sum(bsum);
  if (ps.bias_part && lane == 0) ps.bias_part[bplace * 4 + w] = bsum;  // side 0 only: each pair counts once
  __syncthreads();
  // 16-byte chunks, rows contiguous, as xview_side_coef_kernel
  constexpr int kCpr = kXvTile * (int)sizeof(T) / 16;
  constexpr int kCpp = kCpr * kXvTile;
  char* gt = p.gbuf + (long long)I * kXvTile * p.ldg + (long long)J * kXvTile * (int)sizeof(T);
#pragma unroll
  for (int c = 0; c < kTile128Lds / 16 / kXvThreads; ++c) {
    const int idx = c * kXvThreads + tid;
    const int plane = idx / kCpp, in = idx - plane * kCpp;
    const int row = in / kCpr, cc = in - row * kCpr;
    const u32x4 v = *reinterpret_cast<const u32x4*>(smem + idx * 16);
    *reinterpret_cast<u32x4*>(gt + plane * p.plane_bytes + (long long)row * p.ldg + cc * 16) = v;
  }
}

// dbias[0] = grad_out[0] * (sum of the `count` partials of C = 2 G) / (2 n). One block: thread t sums
// partials t, t + 1024, ... in order, then a fixed halving tree (fp64): deterministic, no atomics.
__global__ __launch_bounds__(kXvSumThreads) void xview_sigmoid_bias_kernel(const float* __restrict__ part, int count,
                                                                           const float* __restrict__ grad_out,
                                                                           double denom, float* __restrict__ dbias,
                                                                           double* __restrict__ share64) {
  __shared__ double red[kXvSumThreads];
  double t = 0.0;
  for (int i = threadIdx.x; i < count; i += kXvSumThreads) t += (double)part[i];
  red[threadIdx.x] = t;
  __syncthreads();
#pragma unroll
  for (int n = kXvSumThreads / 2; n > 0; n >>= 1) {
    if ((int)threadIdx.x < n) red[threadIdx.x] += red[threadIdx.x + n];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double v = (double)grad_out[0] * red[0] / denom;
    if (dbias) dbias[0] = (float)v;
    else share64[0] = v;
  }
}

}  // namespace dev

namespace {
inline int xv_npad(const Geometry& g) { return roundup(g.rows / 2, dev::kXvTile); }
inline int xv_en(const Geometry& g) { return roundup(g.dim_k, dev::kXvTile); }
inline int xv_planes(DType comp) { return comp == DType::F32 ? 1 : 2; }

// The gathered rows [world * rows_pad][ld_k] as the tile kernels read them (zq may be null: the checks
// alone). A row stage reads 128 rows from local row side * n + I * 128 of the own slot, a column stage
// from (1 - side) * n + Jl * 128 of slot q: at most local row n + n_pad of a slot, so with n + n_pad <=
// rows_pad no stage reads beyond its slot, and none beyond the world * rows_pad rows of the buffer.
dev::XvParams xv_params(DType comp, const void* zq, const Geometry& g, const std::string& who) {
  const UnitRows u = unit_rows(comp, zq, g, who);
  NTXENT_CHECK(g.world >= 1 && g.rank >= 0 && g.rank < g.world, who + ": bad world / rank");
  NTXENT_CHECK(u.ldb % 16 == 0, who + ": geometry does not pad K to 128 bytes");
  const int n = g.rows / 2, np = xv_npad(g);
  NTXENT_CHECK(n + np <= g.rows_pad, who + ": a 128-row stage would leave its rank slot");
  dev::XvParams p{};
  p.zq = u.ptr;
  p.ldb = u.ldb;
  p.n = n;
  p.rows_pad = g.rows_pad;
  p.nk = u.nk;
  p.nT = np / dev::kXvTile;
  p.world = g.world;
  p.rank = g.rank;
  p.nq = g.world;
  p.q_skip = -1;
  p.scale2 = g.inv_temp * dev::kLog2e;
  return p;
}

// One GPU: one rank, whose partials are launch_lse's: rows_pad / 256 slots, which must be the
// n_pad / 128 tiles per side.
dev::XvParams xv_params_one(DType comp, const void* zq, const Geometry& g, const std::string& who) {
  NTXENT_CHECK(g.world == 1, who + ": one rank only (build the geometry with world = 1)");
  const int n = g.rows / 2, np = xv_npad(g);
  NTXENT_CHECK(np <= g.rows_pad && n + np <= g.rows_pad && g.col_tiles == np / dev::kXvTile &&
                   ((size_t)g.ld_k * dtype_size(comp)) % 16 == 0,
               who + ": geometry does not pad rows to 256");
  return xv_params(comp, zq, g, who);
}

// Merge of the world * nT slots into this rank's slot of lse2_all and cpos, then the loss terms' sum
// over the global row count: loss[0] in fp32, or (loss null) share64[0].
void xv_lse_loss(const float2* part, const float* ypos, const Geometry& g, float* lse2_all, float* cpos, double* lpair,
                 float* loss, double* share64, hipStream_t stream) {
  const int n = g.rows / 2, nslots = g.world * (xv_npad(g) / dev::kXvTile);
  hipLaunchKernelGGL(dev::xview_lse_kernel, dim3((n + g.rows_pad - g.rows + 255) / 256), dim3(256), 0, stream, part,
                     ypos, lse2_all + (size_t)g.rank * g.rows_pad, cpos, lpair, n, g.rows_pad, nslots);
  hipLaunchKernelGGL(dev::xview_loss_kernel, dim3(1), dim3(dev::kXvSumThreads), 0, stream, lpair, n,
                     (double)g.global_rows, loss, share64);
}

// The slots [q_lo, q_hi) except q_skip (-1: none) as a forward launch's columns.
void xv_slot_range(dev::XvParams& p, const Geometry& g, int q_lo, int q_hi, int q_skip, const std::string& who) {
  NTXENT_CHECK(0 <= q_lo && q_lo <= q_hi && q_hi <= g.world && q_skip < q_hi && (q_skip < 0 || q_skip >= q_lo),
               who + ": bad slot range");
  p.q_lo = q_lo;
  p.nq = q_hi - q_lo - (q_skip >= 0 ? 1 : 0);
  p.q_skip = q_skip;
}

// kslots: the rank slots that `rows` holds and zt gets side by side, g.world, or 1 (blockIdx.z = v
// then, so the slot strides are never applied).
void xv_launch_zt(DType comp, const void* rows, const Geometry& g, int kslots, void* zt, hipStream_t stream) {
  const int np = xv_npad(g), en = xv_en(g), n = g.rows / 2;
  dispatch_comp(comp, [&](auto tc) {
    using Tc = decltype(tc);
    hipLaunchKernelGGL((dev::xview_transpose_kernel<Tc>), dim3(np / 64, en / 64, 2 * kslots), dim3(256), 0, stream,
                       static_cast<const Tc*>(rows), static_cast<Tc*>(zt), n, g.dim_k, (long long)g.ld_k, en,
                       (long long)kslots * np, (long long)g.rows_pad, (long long)np);
  });
}

// One side's coefficient block in coef: planes of n_pad rows, kslots * n_pad columns.
void xv_coef_planes(DType comp, const Geometry& g, int kslots, void* coef, dev::XvParams& p) {
  p.gbuf = static_cast<char*>(coef);
  p.ldg = (long long)kslots * xv_npad(g) * (long long)dtype_size(comp);
  p.plane_bytes = (long long)xv_npad(g) * p.ldg;
}

void xv_launch_coef(DType comp, dev::XvParams p, const Geometry& g, int side, const float* lse2_all,
                    const float* cpos, void* coef, hipStream_t stream) {
  p.side = side;
  p.lse2 = lse2_all;
  p.cpos = cpos;
  xv_coef_planes(comp, g, g.world, coef, p);
  const int ntiles = p.nT * g.world * p.nT;
  dispatch_comp(comp, [&](auto tc) {
    hipLaunchKernelGGL((dev::xview_side_coef_kernel<decltype(tc)>), dim3(ntiles), dim3(dev::kXvThreads), 0, stream, p);
  });
}

// xview_dz_kernel's arguments with K = world * n_pad per plane: the planes' rows and Zt's rows both
// hold the rank slots side by side, so a plane's K-steps run through the slots in ascending order.
// The dZ tiles write columns [0, En) of rows [side * n, side * n + n) of the [rows_pad][dim_n] slab.
// kslots: the rank slots side by side in a row, g.world, or 1 for the block form (K = n_pad per plane).
dev::XvDzParams xv_dz_params(DType comp, const void* coef, const void* zt, const Geometry& g, float* dz,
                             const std::string& who, int kslots) {
  const size_t es = dtype_size(comp);
  const int np = xv_npad(g), en = xv_en(g);
  NTXENT_CHECK(en <= g.dim_n && ((size_t)np * es) % kKStepBytes == 0, who + ": dim_n < roundup(dim_k, 128)");
  dev::XvDzParams q{};
  q.gbuf = static_cast<const char*>(coef);
  q.ldg = (long long)kslots * np * (long long)es;
  q.plane_bytes = (long long)np * q.ldg;
  q.planes = xv_planes(comp);
  q.zt = static_cast<const char*>(zt);
  q.ldz = q.ldg;
  q.En = en;
  q.n_half = g.rows / 2;
  q.nk = (int)((size_t)q.ldg / kKStepBytes);
  q.out = dz;
  q.ldo = g.dim_n;
  return q;
}
}  // namespace

size_t xview_part_bytes(const Geometry& g) {
  return (size_t)g.world * (xv_npad(g) / dev::kXvTile) * g.rows_pad * sizeof(float2);
}
size_t xview_lse_scratch_bytes(const Geometry& g) { return (size_t)(g.rows / 2) * sizeof(double); }
size_t xview_fwd_scratch_bytes(const Geometry& g) { return xview_part_bytes(g) + xview_lse_scratch_bytes(g); }
// 4 n_pad W n_pad bytes in every plan: 16-bit plans hold two planes, so their coefficients take as
// much as one fp32 block would (twice a single 16-bit G). One side at a time; the caller keeps the
// peak down by releasing zq before the dZ slab and coef / zt before dh, not by a smaller block.
size_t xview_coef_bytes(DType comp, const Geometry& g) {
  return (size_t)xv_planes(comp) * xv_npad(g) * g.world * xv_npad(g) * dtype_size(comp);
}
size_t xview_zt_bytes(DType comp, const Geometry& g) {
  return (size_t)2 * xv_en(g) * g.world * xv_npad(g) * dtype_size(comp);
}
size_t xview_dz_bytes(const Geometry& g) { return (size_t)g.rows_pad * g.dim_n * sizeof(float); }

// ---- one GPU -----------------------------------------------------------------------------------------
void launch_xview_fwd(DType comp, const void* zq, float* ypos, const Geometry& g, float* lse2, float* cpos,
                      float* loss, void* scratch, hipStream_t stream) {
  NTXENT_CHECK(zq && ypos && lse2 && cpos && loss && scratch, "xview_fwd: null buffer");
  dev::XvParams p = xv_params_one(comp, zq, g, "xview_fwd");
  // scratch: the partials [nT][rows_pad] (every entry that is read is written), then the pairs'
  // loss terms [N] (fp64; the partials are a multiple of 8 bytes)
  p.part = static_cast<float2*>(scratch);
  p.ypos = ypos;
  double* lpair = reinterpret_cast<double*>(static_cast<char*>(scratch) + xview_part_bytes(g));
  // side 0's tiles alone: their columns give the view-2 rows' partials
  dispatch_comp(comp, [&](auto tc) {
    hipLaunchKernelGGL((dev::xview_fwd_kernel<decltype(tc), true>), dim3(p.nT * p.nT), dim3(dev::kXvThreads), 0, stream, p);
  });
  xv_lse_loss(p.part, ypos, g, lse2, cpos, lpair, loss, nullptr, stream);
  NTXENT_HIP_CHECK(hipGetLastError());
}

void launch_xview_coef(DType comp, const void* zq, const float* lse2, const float* cpos, const Geometry& g, void* coef,
                       void* zt, hipStream_t stream) {
  NTXENT_CHECK(zq && lse2 && cpos && coef && zt, "xview_coef: null buffer");
  const dev::XvParams p = xv_params_one(comp, zq, g, "xview_coef");
  xv_launch_zt(comp, zq, g, g.world, zt, stream);
  xv_launch_coef(comp, p, g, 0, lse2, cpos, coef, stream);
  NTXENT_HIP_CHECK(hipGetLastError());
}

void launch_xview_dz(DType comp, void* coef, const void* zt, const Geometry& g, float* dz, hipStream_t stream) {
  xv_params_one(comp, nullptr, g, "xview_dz");
  NTXENT_CHECK(coef && zt && dz, "xview_dz: null buffer");
  dev::XvDzParams q = xv_dz_params(comp, coef, zt, g, dz, "xview_dz", g.world);
  const int np = xv_npad(g);
  const dim3 grid(q.En / dev::kXvTile, np / dev::kXvTile);
  dispatch_comp(comp, [&](auto tc) {
    using Tc = decltype(tc);
    // view 1's rows from G, G -> G^T in place, view 2's rows from G^T: both products stream K-major
    // coefficient rows by LDS-DMA
    q.side = 0;
    hipLaunchKernelGGL((dev::xview_dz_kernel<Tc>), grid, dim3(dev::kXvThreads), 0, stream, q);
    hipLaunchKernelGGL((dev::xview_gt_kernel<Tc>), dim3(np / 64, np / 64, q.planes), dim3(256), 0, stream,
                       static_cast<Tc*>(coef), (long long)np, (long long)np * np);
    q.side = 1;
    hipLaunchKernelGGL((dev::xview_dz_kernel<Tc>), grid, dim3(dev::kXvThreads), 0, stream, q);
  });
  NTXENT_HIP_CHECK(hipGetLastError());
}

// ---- pairwise sigmoid loss -----------------------------------------------------------------------------
namespace {
// Rank g.rank's tiles against the rank slots [q_lo, q_hi) except q_skip. rows_q null: the slots are
// zq's, every rank's rows (one: the one-GPU launches' geometry checks, world 1, rows padded to 256).
// Otherwise the block form: zq is the own slot alone and rows_q holds the rows of slot q_lo, the only one.
dev::XvSigParams xv_sig_params(DType comp, const void* zq, const void* rows_q, const Geometry& g, float bias, int q_lo,
                               int q_hi, int q_skip, const float* pos_cos, const std::string& who, bool one = false) {
  dev::XvSigParams ps{};
  ps.x = one ? xv_params_one(comp, zq, g, who) : xv_params(comp, zq, g, who);
  xv_slot_range(ps.x, g, q_lo, q_hi, q_skip, who);
  NTXENT_CHECK(!rows_q || ps.x.nq == 1, who + ": a block is one slot");
  ps.x.zcol = static_cast<const char*>(rows_q);
  ps.scale2 = (double)g.inv_temp * 1.4426950408889634;
  ps.bias2 = (double)bias * 1.4426950408889634;
  ps.pos_cos = rows_q && q_lo != g.rank ? nullptr : pos_cos;  // the own block alone holds positives
  return ps;
}
// side 0's tiles of a rank: nT row tiles x world * nT column tiles
inline size_t xv_sig_tiles(const Geometry& g) {
  const size_t nT = (size_t)(xv_npad(g) / dev::kXvTile);
  return nT * (size_t)g.world * nT;
}
// block: the kBlock form (the columns are ps.x.zcol's rows)
void xv_sig_launch_fwd(DType comp, dev::XvSigParams ps, double* lpart, bool block, hipStream_t stream) {
  ps.lpart = lpart;
  const dim3 grid(ps.x.nT * ps.x.nq * ps.x.nT);
  dispatch_comp(comp, [&](auto tc) {
    using Tc = decltype(tc);
    if (!block) {
      hipLaunchKernelGGL((dev::xview_sigmoid_fwd_kernel<Tc>), grid, dim3(dev::kXvThreads), 0, stream, ps);
    } else {
      hipLaunchKernelGGL((dev::xview_sigmoid_fwd_kernel<Tc, true>), grid, dim3(dev::kXvThreads), 0, stream, ps);
    }
  });
}
// one side's block against ps's slots into coef (xv_coef_planes); bias_part with side 0 and only there
void xv_sig_launch_coef(DType comp, dev::XvSigParams ps, const Geometry& g, int side, void* coef, float* bias_part,
                        bool block, hipStream_t stream) {
  ps.x.side = side;
  xv_coef_planes(comp, g, ps.x.nq, coef, ps.x);
  ps.bias_part = bias_part;
  const dim3 grid(ps.x.nT * ps.x.nq * ps.x.nT);
  dispatch_comp(comp, [&](auto tc) {
    using Tc = decltype(tc);
    if (!block) {
      hipLaunchKernelGGL((dev::xview_sigmoid_coef_kernel<Tc>), grid, dim3(dev::kXvThreads), 0, stream, ps);
    } else {
      hipLaunchKernelGGL((dev::xview_sigmoid_coef_kernel<Tc, true>), grid, dim3(dev::kXvThreads), 0, stream, ps);
    }
  });
}
}  // namespace

size_t xview_sigmoid_scratch_bytes(const Geometry& g) { return xv_sig_tiles(g) * sizeof(double); }
size_t xview_sigmoid_bias_part_bytes(const Geometry& g) { return xv_sig_tiles(g) * 4 * sizeof(float); }

void launch_xview_sigmoid_pos(DType in, const void* h, const float* inv, const Geometry& g, float* pos_cos,
                              hipStream_t stream) {
  NTXENT_CHECK(h && inv && pos_cos, "xview_sigmoid_pos: null buffer");
  NTXENT_CHECK(in != DType::FP8, "xview_sigmoid_pos: fp32 | fp16 | bf16 rows");
  const int n = g.rows / 2;
  dispatch_comp(in, [&](auto tin) {
    using Tin = decltype(tin);
    hipLaunchKernelGGL((dev::xview_sigmoid_pos_kernel<Tin>), dim3((n + 3) / 4), dim3(256), 0, stream,
                       static_cast<const Tin*>(h), inv, pos_cos, n, g.dim);
  });
  NTXENT_HIP_CHECK(hipGetLastError());
}

void launch_xview_sigmoid_fwd(DType comp, const void* zq, const Geometry& g, float bias, float* loss, void* scratch,
                              hipStream_t stream, const float* pos_cos) {
  NTXENT_CHECK(zq && loss && scratch, "xview_sigmoid_fwd: null buffer");
  double* lpart = static_cast<double*>(scratch);
  xv_sig_launch_fwd(comp, xv_sig_params(comp, zq, nullptr, g, bias, 0, 1, -1, pos_cos, "xview_sigmoid_fwd", true), lpart,
                    false, stream);
  // the tiles' partials in a fixed order, over the n pairs
  hipLaunchKernelGGL(dev::xview_loss_kernel, dim3(1), dim3(dev::kXvSumThreads), 0, stream, lpart, (int)xv_sig_tiles(g),
                     (double)(g.rows / 2), loss, nullptr);
  NTXENT_HIP_CHECK(hipGetLastError());
}

void launch_xview_sigmoid_coef(DType comp, const void* zq, const Geometry& g, float bias, void* coef, void* zt,
                               float* bias_part, hipStream_t stream, const float* pos_cos) {
  NTXENT_CHECK(zq && coef && zt && bias_part, "xview_sigmoid_coef: null buffer");
  const dev::XvSigParams ps = xv_sig_params(comp, zq, nullptr, g, bias, 0, 1, -1, pos_cos, "xview_sigmoid_coef", true);
  xv_launch_zt(comp, zq, g, g.world, zt, stream);
  xv_sig_launch_coef(comp, ps, g, 0, coef, bias_part, false, stream);
  NTXENT_HIP_CHECK(hipGetLastError());
}

void launch_xview_sigmoid_bias_grad(const float* bias_part, const float* grad_out, float* dbias, const Geometry& g,
                                    hipStream_t stream, double* share64) {
  NTXENT_CHECK(bias_part && grad_out && (dbias != nullptr) != (share64 != nullptr),
               "xview_sigmoid_bias_grad: null buffer (one of dbias and share64)");
  // 2 N: the rows of the global batch (one GPU: 2 n)
  hipLaunchKernelGGL(dev::xview_sigmoid_bias_kernel, dim3(1), dim3(dev::kXvSumThreads), 0, stream, bias_part,
                     (int)(4 * xv_sig_tiles(g)), grad_out, (double)g.global_rows, dbias, share64);
  NTXENT_HIP_CHECK(hipGetLastError());
}

// ---- rank g.rank of g.world: every slot gathered in zq (rows_q null, kslots = g.world), or the block
// form, ONE rank slot at a time (the ring exchange; rows_q, kslots = 1) ------------------------------------
// Block form: zq is this rank's own slot [rows_pad][ld_k]; rows_q a buffer of the same shape that holds
// rank q's rows (q == g.rank: zq itself). Every row a stage can read, up to local row n + n_pad <=
// rows_pad, lies in the one slot: the buffers must be whole slots (received whole, or zero beyond what
// was received). Nothing there has a size that depends on g.world except lpart / bias_part, which keep
// the gather launches' layout so that the same two sums finish the loss and dL/dbias.
void launch_xview_sigmoid_dist_fwd(DType comp, const void* zq, const void* rows_q, const Geometry& g, float bias,
                                   int q_lo, int q_hi, int q_skip, double* lpart, hipStream_t stream,
                                   const float* pos_cos) {
  NTXENT_CHECK(zq && lpart, "xview_sigmoid_dist_fwd: null buffer");
  const dev::XvSigParams ps =
      xv_sig_params(comp, zq, rows_q, g, bias, q_lo, q_hi, q_skip, pos_cos, "xview_sigmoid_dist_fwd");
  if (ps.x.nq == 0) return;
  xv_sig_launch_fwd(comp, ps, lpart, rows_q != nullptr, stream);
  NTXENT_HIP_CHECK(hipGetLastError());
}

void launch_xview_sigmoid_dist_loss(const double* lpart, const Geometry& g, double* share, hipStream_t stream) {
  NTXENT_CHECK(lpart && share, "xview_sigmoid_dist_loss: null buffer");
  hipLaunchKernelGGL(dev::xview_loss_kernel, dim3(1), dim3(dev::kXvSumThreads), 0, stream, lpart, (int)xv_sig_tiles(g),
                     (double)(g.global_rows / 2), nullptr, share);
  NTXENT_HIP_CHECK(hipGetLastError());
}

void launch_xview_sigmoid_dist_coef(DType comp, const void* zq, const void* rows_q, int q, const Geometry& g, float bias,
                                    int side, void* coef, float* bias_part, hipStream_t stream, const float* pos_cos) {
  NTXENT_CHECK(zq && coef && (side == 0 || side == 1), "xview_sigmoid_dist_coef: bad argument");
  NTXENT_CHECK((side == 0) == (bias_part != nullptr), "xview_sigmoid_dist_coef: bias_part with side 0 and only there");
  const dev::XvSigParams ps = xv_sig_params(comp, zq, rows_q, g, bias, rows_q ? q : 0, rows_q ? q + 1 : g.world, -1,
                                            pos_cos, "xview_sigmoid_dist_coef");
  xv_sig_launch_coef(comp, ps, g, side, coef, bias_part, rows_q != nullptr, stream);
  NTXENT_HIP_CHECK(hipGetLastError());
}

void launch_xview_dist_fwd(DType comp, const void* zq_all, const Geometry& g, int q_lo, int q_hi, int q_skip,
                           float2* part, float* ypos, hipStream_t stream) {
  NTXENT_CHECK(zq_all && part && ypos, "xview_dist_fwd: null buffer");
  dev::XvParams p = xv_params(comp, zq_all, g, "xview_dist_fwd");
  xv_slot_range(p, g, q_lo, q_hi, q_skip, "xview_dist_fwd");
  p.part = part;
  p.ypos = ypos;
  if (p.nq == 0) return;
  const int ntiles = 2 * p.nT * p.nq * p.nT;
  dispatch_comp(comp, [&](auto tc) {
    hipLaunchKernelGGL((dev::xview_fwd_kernel<decltype(tc), false>), dim3(ntiles), dim3(dev::kXvThreads), 0, stream, p);
  });
  NTXENT_HIP_CHECK(hipGetLastError());
}

void launch_xview_dist_lse(const float2* part, const float* ypos, const Geometry& g, float* lse2_all, float* cpos,
                           double* loss, void* scratch, hipStream_t stream) {
  NTXENT_CHECK(part && ypos && lse2_all && cpos && loss && scratch, "xview_dist_lse: null buffer");
  xv_lse_loss(part, ypos, g, lse2_all, cpos, static_cast<double*>(scratch), nullptr, loss, stream);
  NTXENT_HIP_CHECK(hipGetLastError());
}

void launch_xview_dist_zt(DType comp, const void* rows, const Geometry& g, int kslots, void* zt, hipStream_t stream) {
  NTXENT_CHECK(rows && zt && (kslots == g.world || kslots == 1), "xview_dist_zt: bad argument");
  xv_params(comp, rows, g, "xview_dist_zt");
  xv_launch_zt(comp, rows, g, kslots, zt, stream);
  NTXENT_HIP_CHECK(hipGetLastError());
}

void launch_xview_dist_coef(DType comp, const void* zq_all, const float* lse2_all, const float* cpos,
                            const Geometry& g, int side, void* coef, hipStream_t stream) {
  NTXENT_CHECK(zq_all && lse2_all && cpos && coef && (side == 0 || side == 1), "xview_dist_coef: bad argument");
  xv_launch_coef(comp, xv_params(comp, zq_all, g, "xview_dist_coef"), g, side, lse2_all, cpos, coef, stream);
  NTXENT_HIP_CHECK(hipGetLastError());
}

void launch_xview_dist_dz(DType comp, const void* coef, const void* zt, const Geometry& g, int kslots, int side,
                          float* dz, bool accumulate, hipStream_t stream) {
  NTXENT_CHECK(coef && zt && dz && (side == 0 || side == 1) && (kslots == g.world || kslots == 1),
               "xview_dist_dz: bad argument");
  xv_params(comp, nullptr, g, "xview_dist_dz");
  dev::XvDzParams q = xv_dz_params(comp, coef, zt, g, dz, "xview_dist_dz", kslots);
  q.side = side;
  const dim3 grid(q.En / dev::kXvTile, xv_npad(g) / dev::kXvTile);
  dispatch_comp(comp, [&](auto tc) {
    using Tc = decltype(tc);
    if (accumulate) {
      hipLaunchKernelGGL((dev::xview_dz_kernel<Tc, true>), grid, dim3(dev::kXvThreads), 0, stream, q);
    } else {
      hipLaunchKernelGGL((dev::xview_dz_kernel<Tc, false>), grid, dim3(dev::kXvThreads), 0, stream, q);
    }
  });
  NTXENT_HIP_CHECK(hipGetLastError());
}

size_t xview_block_coef_bytes(DType comp, const Geometry& g) {
  return (size_t)xv_planes(comp) * xv_npad(g) * xv_npad(g) * dtype_size(comp);
}
size_t xview_block_zt_bytes(DType comp, const Geometry& g) {
  return (size_t)2 * xv_en(g) * xv_npad(g) * dtype_size(comp);
}

}  // namespace ntxent
