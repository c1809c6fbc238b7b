// Cross-view retrieval-rank kernels for gfx950: in-batch two-tower retrieval (where a view-1 row's
// partner ranks among the N view-2 rows, and the other way round) and each row's hardest in-batch
// negative, without any N^2 data in memory.
//
// zq: launch_prep's unit rows [view 1 (n); view 2 (n); pad], a_i = zq_i, b_i = zq_(n + i), and
// S = A B^T (fp32 MFMA sums). Outputs in stacked order, entry i: a_i ranked among b, entry n + i:
// b_i ranked among a:
//   pos_cos[i] = pos_cos[n + i] = t_i = <a_i, b_i>
//   rank[i]     = #{ j != i : S_ij > t_i }        (row i of S)
//   rank[n + i] = #{ j != i : S_ji > t_i }        (column i of S)
//   hard_neg_cos / hard_neg_index: the largest S over the same j and the lowest j that attains it
//   (-inf / -1 when n == 1)
//
//   xview_rank_init   : a wave per pair: t_i (fp32 dot over the stored rows, fixed lane tree),
//                       rank = 0, the hardest-negative keys = 0 ("none").
//   xview_rank_kernel : one 128 x 128 tile (I, J) of S per workgroup over the full nT x nT grid
//                       (xcd_remap order) by tile128.h's MFMA loop; A from row I * 128, B from row
//                       n + J * 128 (not tile aligned). The epilogue treats the tile twice: its rows
//                       against t of the rows (the columns are the candidates), and its columns
//                       against t of the columns (the rows are the candidates). Counts are packed
//                       one per byte; a maximum travels with the candidate's index, and every
//                       reduction step (lane, DPP row, wave pair, tiles) keeps the lower index on a
//                       tie. Per row / column and tile ONE integer atomic add merges the count and
//                       ONE 64-bit unsigned atomic max the key
//                         (order-preserving image of the cosine, unsigned) << 32 | 0xffffffff - index,
//                       so any arrival order leaves the same bits. No float atomics.
//   xview_rank_finish : the keys unpacked into hard_neg_cos and hard_neg_index.
#include "../include/ntxent/ntxent.h"
#include "device_common.h"
#include "host_common.h"
#include "rank_common.h"
#include "tile128.h"

namespace ntxent {
namespace dev {

constexpr int kXrTile = kTile128;
constexpr int kXrNoIndex = 0x7fffffff;  // above every candidate index: loses every tie

struct XrParams {
  const char* zq;  // [rows_pad][ldb bytes] unit rows (zero K padding, zero pad rows)
  long long ldb;   // row stride in bytes
  int n;           // pairs
  int nk;          // 128-byte K-steps per row
  int nT;          // 128-row tiles per view
  int* rank;       // [2n]
  float* pos;      // [2n]
  unsigned long long* key;  // [2n] hardest-negative keys, 0: no negative seen
};

// (cosine, candidate index) as an unsigned key: a larger cosine gives a larger key, equal cosines
// the larger key to the lower index. -0 is folded into +0 first: the two compare equal as floats
// and must not differ in the key. Every key of a real cosine is above 0, the "none" key.
__device__ __forceinline__ unsigned long long xr_key(float v, int idx) {
  const unsigned hi = (unsigned)f2ord(v + 0.f) ^ 0x80000000u;
  return ((unsigned long long)hi << 32) | (0xffffffffu - (unsigned)idx);
}

// minimum over the 16 lanes of a DPP row (every lane gets it)
__device__ __forceinline__ int row16_imin(int x) {
  x = min(x, dpp_i<0x128>(x));
  x = min(x, dpp_i<0x124>(x));
  x = min(x, dpp_i<0x122>(x));
  x = min(x, dpp_i<0x121>(x));
  return x;
}

// ---- prologue: positive cosines and output initialisation -------------------------------
// One wave per pair (i, i + n); lane l sums the 16-byte chunks l, l + 64, ... of the two rows
// (pos_rank_init_kernel's addressing and summation order).
template <typename T>
__global__ __launch_bounds__(256) void xview_rank_init_kernel(const XrParams p, int chunks) {
  constexpr int E = 16 / (int)sizeof(T);
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= p.n) return;
  const char* a = p.zq + (long long)i * p.ldb;
  const char* b = p.zq + (long long)(i + p.n) * p.ldb;
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
    const int r = i + lane * p.n;
    p.pos[r] = s;
    p.rank[r] = 0;
    p.key[r] = 0ull;
  }
}

__global__ __launch_bounds__(256) void xview_rank_finish_kernel(const unsigned long long* __restrict__ key,
                                                                float* __restrict__ hard, int* __restrict__ index,
                                                                int rows) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  const unsigned long long k = key[i];
  hard[i] = k ? ord2f((int)((unsigned)(k >> 32) ^ 0x80000000u)) : kNegInf;
  index[i] = k ? (int)(0xffffffffu - (unsigned)k) : -1;
}

// ---- the tile kernel ---------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kTile128Threads) void xview_rank_kernel(const XrParams p) {
  // ONE __shared__ object (staging ring, reused by the epilogue): see small_bwd_kernel
  __shared__ __attribute__((aligned(16))) char smem[kTile128Lds];
  lds_char* lds = (lds_char*)smem;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, r16 = lane & 15, g = lane >> 4;
  const int n = p.n;

  const int b = xcd_remap(blockIdx.x, gridDim.x);
  const int I = b / p.nT, J = b - I * p.nT;

  // A = view-1 rows of tile I, B = view-2 rows of tile J (from row n on: not tile aligned)
  const char* arow = p.zq + (long long)I * kXrTile * p.ldb;
  const char* brow = p.zq + ((long long)n + (long long)J * kXrTile) * p.ldb;
  f32x4 acc[4][4];
  tile128_gemm<T>(
      lds, p.nk, [&](int k) { return Tile128Src{arow + (long long)k * kKStepBytes, p.ldb}; },
      [&](int k) { return Tile128Src{brow + (long long)k * kKStepBytes, p.ldb}; }, false, Tile128Plain{}, acc);

  // epilogue LDS over the staging images: t of the tile's rows and columns | per-wave-column row
  // (count, max, index) | per-wave-row column (count, max, index)
  float* s_t = reinterpret_cast<float*>(smem);         // [256]: rows, then columns
  int* s_rc = reinterpret_cast<int*>(s_t + 256);       // [2][128]
  float* s_rm = reinterpret_cast<float*>(s_rc + 256);  // [2][128]
  int* s_ri = reinterpret_cast<int*>(s_rm + 256);      // [2][128]
  int* s_cc = s_ri + 256;                              // [2][128]
  float* s_cm = reinterpret_cast<float*>(s_cc + 256);  // [2][128]
  int* s_ci = reinterpret_cast<int*>(s_cm + 256);      // [2][128]
  {
    // a pair's threshold is the same in both directions: pos[li] == pos[n + li]
    const int li = (tid < kXrTile ? I * kXrTile : J * kXrTile - kXrTile) + tid;
    s_t[tid] = li < n ? p.pos[li] : 0.f;
  }
  __syncthreads();

  // counts of 4 rows (r) / 4 columns (ni) packed one per byte: at most 64 per wave and entry
  int cnt_r[4] = {0, 0, 0, 0}, cnt_c = 0;
  float mx_r[4][4], mx_c[4], tc[4];
  int ix_r[4][4], ix_c[4], gj[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int ct = 64 * wc + 16 * ni + r16;
    gj[ni] = J * kXrTile + ct;
    tc[ni] = s_t[kXrTile + ct];
    mx_c[ni] = kNegInf;
    ix_c[ni] = kXrNoIndex;
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rt = 64 * wr + 16 * mi + 4 * g + r;
      const int gi = I * kXrTile + rt;
      const float ti = s_t[rt];
      float m = kNegInf;
      int ix = kXrNoIndex;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const float v = acc[mi][ni][r];
        // pair indices at or beyond n are the other view's rows or padding: masked by index, as
        // is the pair's own positive
        const bool ok = (gi < n) & (gj[ni] < n) & (gi != gj[ni]);
        cnt_r[mi] += (int)(ok & (v > ti)) << (8 * r);
        cnt_c += (int)(ok & (v > tc[ni])) << (8 * ni);
        const float vm = ok ? v : kNegInf;
        // a lane meets its columns (ni) and its rows (mi, r) in ascending order: the strict
        // compare keeps the lowest index of equal values
        if (vm > m) {
          m = vm;
          ix = gj[ni];
        }
        if (vm > mx_c[ni]) {
          mx_c[ni] = vm;
          ix_c[ni] = gi;
        }
      }
      const float mr = row16_max(m);
      mx_r[mi][r] = mr;
      ix_r[mi][r] = row16_imin(m == mr ? ix : kXrNoIndex);
    }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) cnt_r[mi] = row16_isum(cnt_r[mi]);
  cnt_c += __shfl_xor(cnt_c, 16, 64);
  cnt_c += __shfl_xor(cnt_c, 32, 64);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const float mc = xrow_max(mx_c[ni]);
    int ic = mx_c[ni] == mc ? ix_c[ni] : kXrNoIndex;
    ic = min(ic, __shfl_xor(ic, 16, 64));
    ic = min(ic, __shfl_xor(ic, 32, 64));
    mx_c[ni] = mc;
    ix_c[ni] = ic;
  }
  if (r16 == 0) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rt = 64 * wr + 16 * mi + 4 * g + r;
        s_rc[wc * kXrTile + rt] = (cnt_r[mi] >> (8 * r)) & 0xff;
        s_rm[wc * kXrTile + rt] = mx_r[mi][r];
        s_ri[wc * kXrTile + rt] = ix_r[mi][r];
      }
  }
  if (g == 0) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int ct = 64 * wc + 16 * ni + r16;
      s_cc[wr * kXrTile + ct] = (cnt_c >> (8 * ni)) & 0xff;
      s_cm[wr * kXrTile + ct] = mx_c[ni];
      s_ci[wr * kXrTile + ct] = ix_c[ni];
    }
  }
  __syncthreads();
  // threads [0, 128): the tile's rows -> entries of view 1; [128, 256): its columns -> view 2.
  // The second wave of a pair holds the higher candidate indices: it wins only a strictly larger
  // maximum.
  {
    const bool col = tid >= kXrTile;
    const int t = tid & (kXrTile - 1);
    const int li = (col ? J : I) * kXrTile + t;
    if (li < n) {
      const int* sc = col ? s_cc : s_rc;
      const float* sm = col ? s_cm : s_rm;
      const int* si = col ? s_ci : s_ri;
      const int c = sc[t] + sc[kXrTile + t];
      const bool second = sm[kXrTile + t] > sm[t];
      const float m = second ? sm[kXrTile + t] : sm[t];
      const int ix = second ? si[kXrTile + t] : si[t];
      const int e = (col ? n : 0) + li;
      if (c) __hip_atomic_fetch_add(p.rank + e, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (m > kNegInf) __hip_atomic_fetch_max(p.key + e, xr_key(m, ix), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace dev

size_t xview_rank_scratch_bytes(const Geometry& g) { return (size_t)g.rows * sizeof(unsigned long long); }

void launch_xview_rank(DType comp, const void* zq, const Geometry& g, int* rank, float* pos_cos, float* hard_neg_cos,
                       int* hard_neg_index, void* key_scratch, hipStream_t stream) {
  NTXENT_CHECK(g.world == 1, "xview_rank: one rank only (build the geometry with world = 1)");
  NTXENT_CHECK(g.rows >= 2 && g.rows % 2 == 0, "xview_rank: two stacked views");
  const UnitRows u = unit_rows(comp, zq, g, "xview_rank");
  NTXENT_CHECK(u.ldb % 16 == 0, "xview_rank: geometry does not pad K to 128 bytes");
  NTXENT_CHECK(key_scratch != nullptr && reinterpret_cast<uintptr_t>(key_scratch) % 8 == 0,
               "xview_rank: key_scratch must be 8-byte aligned");
  dev::XrParams p{};
  p.zq = u.ptr;
  p.ldb = u.ldb;
  p.n = g.rows / 2;
  p.nk = u.nk;
  p.nT = (p.n + dev::kXrTile - 1) / dev::kXrTile;
  p.rank = rank;
  p.pos = pos_cos;
  p.key = static_cast<unsigned long long*>(key_scratch);
  // the tile kernel reads rows [0, nT * 128) as A and rows [n, n + nT * 128) as B
  NTXENT_CHECK(p.n + p.nT * dev::kXrTile <= g.rows_pad, "xview_rank: a 128-row stage would leave the unit rows");
  const int chunks = u.nk * (kKStepBytes / 16);
  dispatch_comp(comp, [&](auto tc) {
    using Tc = decltype(tc);
    hipLaunchKernelGGL((dev::xview_rank_init_kernel<Tc>), dim3((p.n + 3) / 4), dim3(256), 0, stream, p, chunks);
    hipLaunchKernelGGL((dev::xview_rank_kernel<Tc>), dim3(p.nT * p.nT), dim3(dev::kTile128Threads), 0, stream, p);
  });
  hipLaunchKernelGGL(dev::xview_rank_finish_kernel, dim3((g.rows + 255) / 256), dim3(256), 0, stream, p.key,
                     hard_neg_cos, hard_neg_index, g.rows);
  NTXENT_HIP_CHECK(hipGetLastError());
}

}  // namespace ntxent
