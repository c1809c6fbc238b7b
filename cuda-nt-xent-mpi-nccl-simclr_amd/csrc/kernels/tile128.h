// The 128 x 128 MFMA tile loop of the positive-rank and cross-view kernels (rank_kernels.hip,
// xview_kernels.hip): acc = A B^T over K-major operand rows, one tile per workgroup. 4 waves, 64 x 64
// each (4 x 4 MFMA blocks of 16 x 16), fp32 accumulators; both operands staged 128 B of K per row
// per step by global_load_lds into a double-buffered, XOR-swizzled LDS image. Device code only.
#pragma once
#include "../include/ntxent/ntxent.h"
#include "device_common.h"

namespace ntxent {
namespace dev {

constexpr int kTile128 = 128;
constexpr int kTile128Threads = 256;
constexpr int kTile128Stage = kTile128 * kKStepBytes;  // LDS bytes of one operand's K-step (16 KiB)
constexpr int kTile128Lds = 4 * kTile128Stage;         // two buffers of an A and a B image

// LDS image of a [128 rows][128 B] K-step: 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7).
// Two rows share a 256-byte bank row, so the 16 rows x one chunk of a ds_read_b128 lane group
// (rows 0-3 and 12-15 at chunk c, rows 4-11 at chunk c ^ 1) land on 16 different 16-byte slots.
__device__ __forceinline__ int tile128_off(int row, int chunk) {
  return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

// K-step bytes [0, 128) of 128 operand rows: row r at ptr + r * ld.
struct Tile128Src {
  const char* ptr;
  long long ld;
};

// Stage one K-step of 128 rows into `dst`: every wave moves 4 pieces of 1 KiB (8 rows); LDS is
// written lane-linear, the swizzle is applied on the source address.
__device__ __forceinline__ void tile128_stage(Tile128Src src, lds_char* dst, int w, int lane) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int piece = w * 4 + q;
    const int row = piece * 8 + (lane >> 3);
    const int lc = (lane & 7) ^ ((row >> 1) & 7);
    __builtin_amdgcn_global_load_lds((const void*)(src.ptr + (long long)row * src.ld + lc * 16),
                                     (lds_void*)(dst + piece * 1024), 16, 0, 0);
  }
}

// One K-step of the tile from the staged images: 4 x 4 MFMA blocks of 16 x 16 per wave.
template <typename T>
__device__ __forceinline__ void tile128_mma_step(const lds_char* aimg, const lds_char* bimg, int wr, int wc, int r16,
                                                 int g, f32x4 (&acc)[4][4]) {
  typedef typename Mfma<T>::frag frag;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    frag a[4], bf[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
      a[mi] = *(__attribute__((address_space(3))) const frag*)(aimg + tile128_off(64 * wr + 16 * mi + r16, 4 * ks + g));
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      bf[ni] = *(__attribute__((address_space(3))) const frag*)(bimg + tile128_off(64 * wc + 16 * ni + r16, 4 * ks + g));
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = Mfma<T>::mma(a[mi], bf[ni], acc[mi][ni]);
  }
}

// acc = sum over steps k in [0, nsteps), ascending, of A_k B_k^T, with a_at(k) / b_at(k) the
// Tile128Src of step k's operand rows. `lds`: kTile128Lds bytes; buffer s holds its A image at
// s * 2 * kTile128Stage and its B image behind it. same_ab (block-uniform): B is A; one image is
// staged and read as both operands and b_at is not called. on_step(k, acc) runs before the
// multiply of step k. kEndBarrier: end with a block barrier, after which the caller may reuse
// `lds`; a caller that does not touch LDS again can do without.
template <typename T, bool kEndBarrier = true, class AAt, class BAt, class OnStep>
__device__ __forceinline__ void tile128_gemm(lds_char* lds, int nsteps, AAt a_at, BAt b_at, bool same_ab,
                                             OnStep on_step, f32x4 (&acc)[4][4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wr = w >> 1, wc = w & 1, r16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  // step k into the buffer at byte offset `buf`: its A image, and its B image behind it
  const auto stage = [&](int k, int buf) {
    tile128_stage(a_at(k), lds + buf, w, lane);
    if (!same_ab) tile128_stage(b_at(k), lds + buf + kTile128Stage, w, lane);
  };
  stage(0, 0);
  for (int k = 0, buf = 0; k < nsteps; ++k, buf ^= 2 * kTile128Stage) {
    // step k landed for this wave; the raw barrier (no further vmcnt drain) makes it visible to
    // every wave and orders every wave's reads of step k - 1 (lgkmcnt) before its slot is restaged
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (k + 1 < nsteps) stage(k + 1, buf ^ 2 * kTile128Stage);
    on_step(k, acc);
    const lds_char* aimg = lds + buf;
    tile128_mma_step<T>(aimg, same_ab ? aimg : aimg + kTile128Stage, wr, wc, r16, g, acc);
  }
  if constexpr (kEndBarrier) __syncthreads();  // every wave is done with the staging images
}

// No work between the steps: the on_step of a plain product.
struct Tile128Plain {
  __device__ __forceinline__ void operator()(int, f32x4 (&)[4][4]) const {}
};

}  // namespace dev
}  // namespace ntxent
