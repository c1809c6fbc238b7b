// ntxent-mi355x — the symmetric data-parallel step: its schedule, its buffers and its launches, once.
//
// Symmetric negatives: every unordered rank pair's similarity block is computed ONCE across the
// group. The computing rank keeps row AND column partials of its cross tiles, forms both
// coefficient blocks C_{r,q} and C_{q,r} = C_{r,q}^T from its kept cosines, and produces the
// partner's gradient contribution C_{q,r} Z_r, which travels back point to point.
//
// Three drivers run this step: the native Engine (engine_sym.cpp, over Comm::send_recv), the
// autograd op (parallel/symmetric.py, over torch.distributed) and the one-GPU emulation
// (parallel/emulate.py, exchanges as copies). All three walk the SymPlan built here and call the
// phases below between their own exchanges. The assignment, every chunk bound, slot, segment,
// dZ view and buffer size of the symmetric step is computed in sym_step.cpp and nowhere else
// (build_sym_fwd_tiles takes its chunk bounds from sym_chunk_bounds); nothing here knows a
// transport. The counterpart of step.h for world > 1.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>
#include <vector>

#include "ntxent/ntxent.h"

namespace ntxent {

// One message of an exchange, seen from this rank. Which fields count depends on the list:
//   rows / rows_f16 : row tiles [t0, t1) of the sender's rows (rank `peer`'s slot of the gathered
//                     rows when receiving, this rank's when sending);
//   col_partials    : part slots [slot0, slot1) (send: of part_x, receive: of part), columns
//                     [t0, t1) * 256. pack_off < 0: the runs are whole rows, back to back (ONE
//                     contiguous range from slot0); else the k-split block, whose runs are Rpad
//                     apart: pack_off is its float2 offset in a packed scratch of
//                     SymBufferBytes::xsend / xrecv for a driver that packs them;
//   contribs        : row tiles [t0, t1) of contribution slab slot0 (send) / received slab slot0.
// Sends come first in every list; a rank's sends to q and q's receives from it agree in order
// and size.
struct SymXfer {
  bool send;
  int peer;
  int slot0, slot1;
  int t0, t1;
  long long pack_off;
};

// One dZ GEMM of the backward: out[row tiles m0..m1) (+)= A * B. A = coefficient tiles from tile
// a_tile0 of cbuf or mbuf (row panels a_panel_tiles tiles apart), K = k_tiles * 256 columns of
// the ZqT blocks from block b_block0, column b_col0; a K range past one block covers whole
// consecutive blocks (b_kblk_cols columns of each). out: contribution slab `out`, or the own
// slab (out < 0). rows_off: offset of the (m0, m1) tile list in SymPlan::dz_rows.
struct SymDzCall {
  bool mirror;  // A from mbuf (partners' mirrored blocks), else cbuf
  long long a_tile0, a_panel_tiles;
  int b_block0;
  long long b_col0, b_kblk_cols;
  int k_tiles, m0, m1;
  int out;
  bool accum;
  size_t rows_off;
};

// Byte size of every buffer only the symmetric step has.
struct SymBufferBytes {
  size_t sbuf = 0;     // kept cosines, one tile per forward tile
  size_t cbuf = 0;     // own coefficient tiles, compact [row_tiles][c_ld]
  size_t mbuf = 0;     // partners' mirrored blocks [max(1, W/2)][row_tiles][row_tiles] tiles
  size_t part_x = 0;   // column partials of the cross tiles [col_tiles][Rpad] float2
  size_t slab = 0;     // one contribution slab [Rpad][dim_n] on the wire (fp16; fp32 plans: fp32)
  size_t contrib = 0;  // one slab per job
  size_t recv = 0;     // one slab per incoming job (fp32 plans: 0, they follow the own slab)
  size_t own = 0;      // own fp32 slab (fp32 plans: + the received slabs, one stack)
  size_t xsend = 0, xrecv = 0;  // packed column partials of the k-split block
  size_t dz_rows = 0;  // SymPlan::dz_rows
};

// The schedule of one rank: plain data, built once per engine / cached Python plan.
struct SymPlan {
  int world = 1, rank = 0, row_tiles = 0;
  DType bwd = DType::F16;  // dtype of rows, ZqT, cosines, coefficients
  bool f8 = false;         // fp8 forward operand (the fp16 rows travel too: rows_f16)
  bool contrib_f16 = true; // contributions on the wire in fp16 (fp32 plans: fp32)
  std::vector<SymJob> jobs, incoming;  // sym_jobs / sym_incoming
  int nchunks = 1, nfull = 0;          // row chunks; full-block jobs (they precede the split job)
  bool split = false;                  // jobs.back() is the split block
  int n_own = 0, n_fwd = 0, c_ld = 0;  // forward tiles (own block first); cbuf row pitch in tiles
  std::vector<std::pair<int, int>> segs;     // (first, count) of chunk c's cross tiles
  std::vector<std::vector<SymXfer>> rows;    // per chunk
  std::vector<SymXfer> rows_f16, col_partials, contribs;
  std::vector<SymDzCall> partner_dz, own_dz;
  std::vector<int4> dz_rows;  // row-range tile lists of the dZ calls: upload once (SymBuffers::dz_rows)
  SymBufferBytes bytes;
};
SymPlan make_sym_plan(const Geometry& g, DType bwd, bool f8);

// Device pointers of one step; a phase checks the ones it uses.
struct SymBuffers {
  const void* h = nullptr;     // [rows][dim]
  void* zq_all = nullptr;      // gathered unit rows [W][Rpad][ld_k] (bwd dtype), this rank's at slot rank
  void* zq8_all = nullptr;     // gathered e4m3 rows [W][Rpad][ld_k8] (f8)
  void* zqt_all = nullptr;     // ZqT blocks [W][dim_n][ld_t]
  float* inv = nullptr;        // [rows]
  float* ypos = nullptr;       // [rows]
  float2* part = nullptr;      // [col_tiles][Rpad]
  float2* part_x = nullptr;
  void* sbuf = nullptr;
  void* cbuf = nullptr;
  void* mbuf = nullptr;
  float* lse2_all = nullptr;   // [W][Rpad]
  float* cpos = nullptr;       // [Rpad]
  float* block_loss = nullptr; // zero before first use (lse_scratch_floats)
  float* loss = nullptr;       // [1]
  void* contrib = nullptr;
  float* own = nullptr;
  void* recv = nullptr;        // fp16 contributions only
  const int4* fwd_tiles = nullptr;  // build_sym_fwd_tiles(g, plan.jobs, plan.nchunks)
  const int4* dz_rows = nullptr;    // device copy of SymPlan::dz_rows
  const float* grad_out = nullptr;  // device fp32 scalar
  void* dh = nullptr;               // [rows][dim]
};

// The launches, asynchronous on `s`. `ws` carries the reserved-CU count of a launch that
// overlaps a transfer (GemmWorkspace::sched_cus): the driver decides it.
void sym_prep(const SymPlan& p, const Geometry& g, DType in, const SymBuffers& b, hipStream_t s);  // + own transpose
// Forward tiles [first, first + count): the own block is (0, n_own), chunk c's cross tiles segs[c].
void sym_fwd_tiles(const SymPlan& p, const Geometry& g, DType comp, const SymBuffers& b, int first, int count,
                   const GemmWorkspace& ws, hipStream_t s);
void sym_lse(const SymPlan& p, const Geometry& g, const SymBuffers& b, hipStream_t s);
void sym_transpose_partners(const SymPlan& p, const Geometry& g, const SymBuffers& b, hipStream_t s);
void sym_coef(const SymPlan& p, const Geometry& g, const SymBuffers& b, hipStream_t s);
void sym_partner_grads(const SymPlan& p, const Geometry& g, const SymBuffers& b, const GemmWorkspace& ws, hipStream_t s);
void sym_own_grads(const SymPlan& p, const Geometry& g, const SymBuffers& b, const GemmWorkspace& ws, hipStream_t s);
// own + received slabs -> dh: fp16 contributions from b.recv, fp32 ones from the stack in b.own
void sym_norm_bwd(const SymPlan& p, const Geometry& g, DType in, const SymBuffers& b, hipStream_t s);

}  // namespace ntxent
