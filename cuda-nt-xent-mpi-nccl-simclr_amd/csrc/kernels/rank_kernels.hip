// Positive-rank kernels for gfx950: contrastive top-k accuracy of one rank's rows without any
// N^2 data in memory.
//
// For every row i of the unit rows zq (launch_prep's output; R = 2N rows, p(i) = (i + N) mod R):
//   pos_cos[i]      t_i = <zq_i, zq_p(i)>
//   rank[i]         #{ j : j != i, j != p(i), j < R, cos_ij > t_i }   (strict)
//   hard_neg_cos[i] max of cos_ij over the same j (-inf when R == 2)
// The rank does not depend on the temperature and is an integer, so top-k accuracy for any k
// follows from it and its reduction is bitwise repeatable.
//
//   pos_rank_init   : a wave per positive pair: t_i = t_p(i) (fp32 dot over the stored rows, fixed
//                     lane tree), rank = 0, hard_neg_cos = the integer image of -inf.
//   pos_rank_kernel : one 128 x 128 tile of zq zq^T per workgroup over the upper triangle of the
//                     tile grid (xcd_remap order), by tile128.h's MFMA loop; a diagonal tile
//                     stages one operand image and reads it as both. Epilogue:
//                     compare against t, count and take the maximum per row (the tile's columns
//                     are the rows' negatives) and, off the diagonal, per column (the tile's rows
//                     are the columns' negatives: cos is symmetric); counts and maxima are reduced
//                     in the wave (DPP / shuffles), across the waves in LDS, and then merged into
//                     rank / hard_neg_cos by ONE integer atomic add and ONE integer atomic max (on
//                     an order-preserving integer image of the float) per row and tile: repeatable
//                     in any arrival order. No float atomics.
//   pos_rank_finish : hard_neg_cos back from its integer image to fp32, in place.
#include "../include/ntxent/ntxent.h"
#include "device_common.h"
#include "pair_mask.h"
#include "host_common.h"
#include "tile128.h"

namespace ntxent {
namespace dev {

constexpr int kRankTile = kTile128;

struct RankParams {
  const char* zq;   // [rows_pad][ldb bytes] unit rows (zero K padding, zero pad rows)
  long long ldb;    // row stride in bytes
  int R, n_half;
  int nk;           // 128-byte K-steps per row (dim_k * sizeof(T) / 128)
  int nT;           // 128-row tiles per side
  int* rank;        // [R]
  float* pos;       // [R]
  int* hard;        // [R] hard_neg_cos, as its integer image until pos_rank_finish
};

// Order-preserving integer image of a float (signed compare): negative floats are mirrored.
__device__ __forceinline__ int f2ord(float x) {
  const int b = __float_as_int(x);
  return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float ord2f(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

template <int CTRL> __device__ __forceinline__ int dpp_i(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
}
// sum over the 16 lanes of a DPP row (every lane gets it)
__device__ __forceinline__ int row16_isum(int x) {
  x += dpp_i<0x128>(x);
  x += dpp_i<0x124>(x);
  x += dpp_i<0x122>(x);
  x += dpp_i<0x121>(x);
  return x;
}

// ---- prologue: positive cosines and output initialisation -------------------------------
// One wave per pair (i, i + N); lane l sums the 16-byte chunks l, l + 64, ... of the two rows.
template <typename T>
__global__ __launch_bounds__(256) void pos_rank_init_kernel(const RankParams p, int chunks) {
  constexpr int E = 16 / (int)sizeof(T);
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= p.n_half) return;
  const char* a = p.zq + (long long)i * p.ldb;
  const char* b = p.zq + (long long)(i + p.n_half) * p.ldb;
  float s = 0.f;
  for (int c = lane; c < chunks; c += 64) {
    union { u32x4 u; T x[E]; } va, vb;
    va.u = *reinterpret_cast<const u32x4*>(a + c * 16);
    vb.u = *reinterpret_cast<const u32x4*>(b + c * 16);
#pragma unroll
    for (int j = 0; j < E; ++j) s += to_f32<T>(va.x[j]) * to_f32<T>(vb.x[j]);
  }
  s = wave_sum(s);
  if (lane < 2) {
    const int r = i + lane * p.n_half;
    p.pos[r] = s;
    p.rank[r] = 0;
    p.hard[r] = f2ord(kNegInf);
  }
}

__global__ __launch_bounds__(256) void pos_rank_finish_kernel(int* hard, int R) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < R) reinterpret_cast<float*>(hard)[i] = ord2f(hard[i]);
}

// ---- the tile kernel ---------------------------------------------------------------------
// First tile index of tile row I in the row-major upper triangle (diagonal included).
__device__ __forceinline__ int tri_start(int I, int nT) { return I * nT - (I * (I - 1)) / 2; }

template <typename T>
__global__ __launch_bounds__(kTile128Threads) void pos_rank_kernel(const RankParams p) {
  // ONE __shared__ object (staging ring, reused by the epilogue): see small_bwd_kernel
  __shared__ __attribute__((aligned(16))) char smem[kTile128Lds];
  lds_char* lds = (lds_char*)smem;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, r16 = lane & 15, g = lane >> 4;

  // tile (I, J), J >= I, from the remapped block index
  const int b = xcd_remap(blockIdx.x, gridDim.x);
  int I = (int)((2.f * p.nT + 1.f - sqrtf((2.f * p.nT + 1.f) * (2.f * p.nT + 1.f) - 8.f * (float)b)) * 0.5f);
  I = I < 0 ? 0 : (I > p.nT - 1 ? p.nT - 1 : I);
  while (tri_start(I, p.nT) > b) --I;
  while (I + 1 < p.nT && tri_start(I + 1, p.nT) <= b) ++I;
  const int J = I + (b - tri_start(I, p.nT));
  const bool diag = I == J;

  // A = rows of tile I, B = rows of tile J; a diagonal tile stages one image and uses it as both
  const char* arow = p.zq + (long long)I * kRankTile * p.ldb;
  const char* brow = p.zq + (long long)J * kRankTile * p.ldb;
  f32x4 acc[4][4];
  tile128_gemm<T>(
      lds, p.nk, [&](int k) { return Tile128Src{arow + (long long)k * kKStepBytes, p.ldb}; },
      [&](int k) { return Tile128Src{brow + (long long)k * kKStepBytes, p.ldb}; }, diag, Tile128Plain{}, acc);

  // epilogue LDS: t of the tile's rows and columns | per-wave-column row (count, max) | per-wave-row
  // column (count, max)
  float* s_t = reinterpret_cast<float*>(smem);        // [256]: rows, then columns
  int* s_rc = reinterpret_cast<int*>(s_t + 256);      // [2][128]
  float* s_rm = reinterpret_cast<float*>(s_rc + 256);  // [2][128]
  int* s_cc = reinterpret_cast<int*>(s_rm + 256);     // [2][128]
  float* s_cm = reinterpret_cast<float*>(s_cc + 256);  // [2][128]
  {
    const int gr = (tid < kRankTile ? I * kRankTile : J * kRankTile - kRankTile) + tid;
    s_t[tid] = gr < p.R ? p.pos[gr] : 0.f;
  }
  __syncthreads();

  // counts of 4 rows (r) / 4 columns (ni) packed one per byte: at most 64 per wave and entry
  int cnt_r[4] = {0, 0, 0, 0}, cnt_c = 0;
  float mx_r[4][4], mx_c[4], tc[4];
  int gj[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int ct = 64 * wc + 16 * ni + r16;
    gj[ni] = J * kRankTile + ct;
    tc[ni] = s_t[kRankTile + ct];
    mx_c[ni] = kNegInf;
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rt = 64 * wr + 16 * mi + 4 * g + r;
      const int gi = I * kRankTile + rt;
      const float ti = s_t[rt];
      float m = kNegInf;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const float v = acc[mi][ni][r];
        // (pad rows have cosine 0, and are no negatives)
        const bool ok = pair::is_negative(gi, gj[ni], p.R, p.n_half);
        cnt_r[mi] += (int)(ok & (v > ti)) << (8 * r);
        cnt_c += (int)(ok & (v > tc[ni])) << (8 * ni);
        const float vm = ok ? v : kNegInf;
        m = fmaxf(m, vm);
        mx_c[ni] = fmaxf(mx_c[ni], vm);
      }
      mx_r[mi][r] = row16_max(m);
    }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) cnt_r[mi] = row16_isum(cnt_r[mi]);
  cnt_c += __shfl_xor(cnt_c, 16, 64);
  cnt_c += __shfl_xor(cnt_c, 32, 64);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) mx_c[ni] = xrow_max(mx_c[ni]);
  if (r16 == 0) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rt = 64 * wr + 16 * mi + 4 * g + r;
        s_rc[wc * kRankTile + rt] = (cnt_r[mi] >> (8 * r)) & 0xff;
        s_rm[wc * kRankTile + rt] = mx_r[mi][r];
      }
  }
  if (g == 0) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int ct = 64 * wc + 16 * ni + r16;
      s_cc[wr * kRankTile + ct] = (cnt_c >> (8 * ni)) & 0xff;
      s_cm[wr * kRankTile + ct] = mx_c[ni];
    }
  }
  __syncthreads();
  // threads [0, 128): the tile's rows; [128, 256): its columns (a diagonal tile counts rows only)
  {
    const bool col = tid >= kRankTile;
    const int t = tid & (kRankTile - 1);
    const int gr = (col ? J : I) * kRankTile + t;
    if (gr < p.R && !(col && diag)) {
      const int* sc = col ? s_cc : s_rc;
      const float* sm = col ? s_cm : s_rm;
      const int c = sc[t] + sc[kRankTile + t];
      const float m = fmaxf(sm[t], sm[kRankTile + t]);
      if (c) __hip_atomic_fetch_add(p.rank + gr, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (m > kNegInf) __hip_atomic_fetch_max(p.hard + gr, f2ord(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace dev

void launch_pos_rank(DType comp, const void* zq, const Geometry& g, int* rank, float* pos_cos, float* hard_neg_cos,
                     hipStream_t stream) {
  NTXENT_CHECK(g.world == 1, "pos_rank: one rank only (build the geometry with world = 1)");
  const UnitRows u = unit_rows(comp, zq, g, "pos_rank");
  dev::RankParams p{};
  p.zq = u.ptr;
  p.ldb = u.ldb;
  p.R = g.rows;
  p.n_half = g.rows / 2;
  p.nk = u.nk;
  p.nT = (g.rows + dev::kRankTile - 1) / dev::kRankTile;
  p.rank = rank;
  p.pos = pos_cos;
  p.hard = reinterpret_cast<int*>(hard_neg_cos);
  // the tile kernel reads rows [0, nT * 128) of zq
  NTXENT_CHECK(p.nT * dev::kRankTile <= g.rows_pad, "pos_rank: geometry does not pad rows to 128");
  const int chunks = u.nk * (kKStepBytes / 16);
  const int ntiles = p.nT * (p.nT + 1) / 2;
  dispatch_comp(comp, [&](auto tc) {
    using Tc = decltype(tc);
    hipLaunchKernelGGL((dev::pos_rank_init_kernel<Tc>), dim3((p.n_half + 3) / 4), dim3(256), 0, stream, p, chunks);
    hipLaunchKernelGGL((dev::pos_rank_kernel<Tc>), dim3(ntiles), dim3(dev::kTile128Threads), 0, stream, p);
  });
  hipLaunchKernelGGL(dev::pos_rank_finish_kernel, dim3((g.rows + 255) / 256), dim3(256), 0, stream, p.hard, g.rows);
  NTXENT_HIP_CHECK(hipGetLastError());
}

}  // namespace ntxent
