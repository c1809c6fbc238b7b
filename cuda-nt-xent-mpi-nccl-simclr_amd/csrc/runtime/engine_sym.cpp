// Engine: symmetric data-parallel mode (EngineConfig::negatives = Negatives::kSymmetric).
//
// The step itself lives in sym_step.h / sym_step.cpp, the one home of the symmetric step: the
// block assignment, the schedule (SymPlan: chunk segments, exchange lists, dZ calls, buffer
// sizes) and the compute phases, shared with parallel/symmetric.py and parallel/emulate.py. This
// file is the Engine's transport only: it walks the plan's exchange lists over Comm::send_recv on
// the comm stream, with its events, and calls the phases between them.
//
//   forward : prep (+ own ZqT) -> rows point to point in chunks on the comm stream (a peer per
//             xGMI link) while the own upper-triangular tiles run -> each chunk's cross tiles as
//             it lands -> cross tiles' column partials to their rows' owners -> LSE -> LSE
//             all-gather + loss all-reduce.
//   backward: partners' ZqT blocks transposed locally -> coefficient pass -> partners' gradient
//             contributions sent point to point while this rank's own dZ GEMMs run ->
//             normalisation backward summing the received contributions.
// No reference counterpart (the reference has no multi-GPU code).
#include "ntxent/engine.h"
#include "ntxent/trace.h"

namespace ntxent {

void Engine::init_sym() {
  ev_chunk_.resize(sym_.nchunks);
  for (auto& e : ev_chunk_) NTXENT_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (hipEvent_t* e : {&ev_f16_, &ev_x_, &ev_xdone_, &ev_c_, &ev_cdone_})
    NTXENT_HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
}

SymBuffers Engine::sym_buffers(const float* grad_out, void* dh) const {
  SymBuffers b;
  b.h = h_;
  b.zq_all = zq_all_;
  b.zq8_all = zq8_all_;
  b.zqt_all = zqt_all_;
  b.inv = inv_;
  b.ypos = ypos_;
  b.part = part_;
  b.part_x = part_x_;
  b.sbuf = sbuf_;
  b.cbuf = cbuf_;
  b.mbuf = mbuf_;
  b.lse2_all = lse2_all_;
  b.cpos = cpos_;
  b.block_loss = block_loss_;
  b.loss = loss_;
  b.contrib = contrib_;
  b.own = slabs_;
  b.recv = recv_;
  b.fwd_tiles = fwd_tiles_;
  b.dz_rows = dz_rows_;
  b.grad_out = grad_out ? grad_out : one_;
  b.dh = dh;
  return b;
}

void Engine::forward_sym(hipStream_t s) {
  const size_t Rp = g_.rows_pad;
  const SymBuffers b = sym_buffers(nullptr, nullptr);
  sym_prep(sym_, g_, cfg_.input, b, s);
  // rows point to point, chunk c of the row tiles per grouped batch (the cross tiles of chunk c
  // run while chunk c + 1 is on the wire); fp8 plans: the fp16 rows of the backward after them
  auto row_ops = [&](const std::vector<SymXfer>& xs, char* all, size_t row) {
    std::vector<P2POp> ops;
    for (const SymXfer& x : xs)
      ops.push_back({x.send, all + ((size_t)(x.send ? rank_ : x.peer) * Rp + (size_t)x.t0 * kTile) * row,
                     (size_t)(x.t1 - x.t0) * kTile * row, x.peer});
    return ops;
  };
  NTXENT_HIP_CHECK(hipEventRecord(ev_prep_, s));
  NTXENT_HIP_CHECK(hipStreamWaitEvent(comm_stream_, ev_prep_, 0));
  for (int c = 0; c < sym_.nchunks; ++c) {
    const auto ops = row_ops(sym_.rows[c], f8_ ? zq8_all_ : zq_all_, f8_ ? (size_t)g_.ld_k8 : g_.ld_k * cs_);
    if (!ops.empty()) comm_->send_recv(ops, comm_stream_);
    NTXENT_HIP_CHECK(hipEventRecord(ev_chunk_[c], comm_stream_));
  }
  if (f8_) {
    comm_->send_recv(row_ops(sym_.rows_f16, zq_all_, g_.ld_k * cs_), comm_stream_);
    NTXENT_HIP_CHECK(hipEventRecord(ev_f16_, comm_stream_));
  }
  const GemmWorkspace ws_ovl = ws_overlap();
  sym_fwd_tiles(sym_, g_, cfg_.compute, b, 0, sym_.n_own, ws_ovl, s);
  for (int c = 0; c < sym_.nchunks; ++c) {
    NTXENT_HIP_CHECK(hipStreamWaitEvent(s, ev_chunk_[c], 0));
    const bool more = c + 1 < sym_.nchunks || f8_;
    sym_fwd_tiles(sym_, g_, cfg_.compute, b, sym_.segs[c].first, sym_.segs[c].second, more ? ws_ovl : ws_, s);
  }
  if (f8_) NTXENT_HIP_CHECK(hipStreamWaitEvent(s, ev_f16_, 0));
  {
    // column partials of the cross tiles -> their rows' owners. A whole-block message is one
    // contiguous range; the k-split block's runs are packed into xsend_ (one 2-D copy) and
    // unpacked from xrecv_ after the exchange: one op per partner instead of one per row tile
    // (W = 8: 224 -> 8 RCCL ops per step; each op costs the host several microseconds inside the
    // group call).
    NTXENT_TRACE("ntxent.fwd_col_partials");
    std::vector<P2POp> ops;
    const size_t f2 = sizeof(float2);
    std::vector<const SymXfer*> unpack;
    for (const SymXfer& x : sym_.col_partials) {
      const size_t run = (size_t)(x.t1 - x.t0) * kTile;  // float2 per row tile
      const int nm = x.slot1 - x.slot0;
      float2* first = (x.send ? part_x_ : part_) + ((size_t)x.slot0 * Rp + (size_t)x.t0 * kTile);
      float2* wire = x.pack_off < 0 ? first : (x.send ? xsend_ : xrecv_) + x.pack_off;
      if (x.pack_off >= 0 && x.send)
        NTXENT_HIP_CHECK(hipMemcpy2DAsync(wire, run * f2, first, Rp * f2, run * f2, nm, hipMemcpyDeviceToDevice, s));
      if (x.pack_off >= 0 && !x.send) unpack.push_back(&x);
      ops.push_back({x.send, wire, (size_t)nm * run * f2, x.peer});
    }
    NTXENT_HIP_CHECK(hipEventRecord(ev_x_, s));
    NTXENT_HIP_CHECK(hipStreamWaitEvent(comm_stream_, ev_x_, 0));
    comm_->send_recv(ops, comm_stream_);
    NTXENT_HIP_CHECK(hipEventRecord(ev_xdone_, comm_stream_));
    NTXENT_HIP_CHECK(hipStreamWaitEvent(s, ev_xdone_, 0));
    for (const SymXfer* x : unpack) {
      const size_t run = (size_t)(x->t1 - x->t0) * kTile;
      NTXENT_HIP_CHECK(hipMemcpy2DAsync(part_ + ((size_t)x->slot0 * Rp + (size_t)x->t0 * kTile), Rp * f2, xrecv_ + x->pack_off,
                                        run * f2, run * f2, x->slot1 - x->slot0, hipMemcpyDeviceToDevice, s));
    }
  }
  sym_lse(sym_, g_, b, s);
  {
    NTXENT_TRACE("ntxent.lse_gather");
    comm_->all_gather(lse2_all_ + (size_t)rank_ * Rp, lse2_all_, Rp * 4, s);
    comm_->all_reduce_sum(loss_, 1, s);
  }
  if (fault_armed("nonfinite")) NTXENT_HIP_CHECK(hipMemsetAsync(loss_, 0xFF, 4, s));  // NaN
}

void Engine::backward_sym(const float* grad_out, void* dh, hipStream_t s) {
  SymBuffers b = sym_buffers(grad_out, dh);
  sym_transpose_partners(sym_, g_, b, s);
  sym_coef(sym_, g_, b, s);
  sym_partner_grads(sym_, g_, b, ws_, s);
  // point to point: contributions out, the partners' contributions to my rows in (fp32 plans:
  // into the slab stack after the own slab)
  const size_t slab = sym_.bytes.slab, row = slab / g_.rows_pad;
  char* recv = sym_.contrib_f16 ? recv_ : reinterpret_cast<char*>(slabs_) + slab;
  std::vector<P2POp> ops;
  for (const SymXfer& x : sym_.contribs)
    ops.push_back({x.send, (x.send ? contrib_ : recv) + x.slot0 * slab + (size_t)x.t0 * kTile * row,
                   (size_t)(x.t1 - x.t0) * kTile * row, x.peer});
  NTXENT_HIP_CHECK(hipEventRecord(ev_c_, s));
  NTXENT_HIP_CHECK(hipStreamWaitEvent(comm_stream_, ev_c_, 0));
  comm_->send_recv(ops, comm_stream_);
  NTXENT_HIP_CHECK(hipEventRecord(ev_cdone_, comm_stream_));
  sym_own_grads(sym_, g_, b, ws_overlap(), s);  // while the partners' contributions travel
  NTXENT_HIP_CHECK(hipStreamWaitEvent(s, ev_cdone_, 0));
  sym_norm_bwd(sym_, g_, cfg_.input, b, s);
}

}  // namespace ntxent
