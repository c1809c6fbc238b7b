// Native NT-Xent runtime (see include/ntxent/engine.h).
//
// Replaces the reference host launchers ntxent_forward_cuda / ntxent_backward_cuda
// (src/ntxent_kernel.cu:138-203, 205-239): those allocate the 2N x 2N logits, softmax and
// grad_logits per call and run cuBLAS on the legacy stream; here every buffer lives in one
// arena sized once, all work is stream-ordered (graph-capturable) and collectives overlap
// the own-rank tiles.
#include "ntxent/engine.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "ntxent/trace.h"

namespace ntxent {

namespace {

constexpr size_t kAlign = 256;

size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

}  // namespace

Engine::Engine(const EngineConfig& cfg, Comm* comm) : cfg_(cfg), comm_(comm) {
  NTXENT_TRACE("ntxent.engine.init");
  if (cfg.device >= 0) NTXENT_HIP_CHECK(hipSetDevice(cfg.device));
  NTXENT_HIP_CHECK(hipGetDevice(&device_));
  rank_ = comm ? comm->rank() : 0;
  world_ = comm ? comm->world() : 1;
  g_ = make_geometry(cfg.rows, cfg.dim, world_, rank_, cfg.temperature);
  NTXENT_CHECK(!cfg.temperature_grad || world_ == 1, "Engine: temperature_grad needs world == 1");
  f8_ = cfg.compute == DType::FP8;
#ifdef NTXENT_NO_FP8
  if (f8_) throw std::runtime_error("ntxent::Engine: fp8 compute requested but this build has ENABLE_FP8=OFF");
#endif
  if (f8_) cfg_.keep_cos = true;  // fp8: the fp16 backward uses the forward's own cosines
  bwd_ = backward_dtype(cfg.compute);
  cs_ = dtype_size(bwd_);
  symm_ = world_ > 1 && cfg.negatives == Negatives::kSymmetric;
  if (symm_) {
    cfg_.keep_cos = true;  // the coefficient pass reads both blocks' cosines from the forward
    sym_ = make_sym_plan(g_, bwd_, f8_);
  }
  ws_.num_cus = device_info(device_).num_cus;
  ov_.small_path = cfg.small_path;
  ov_.small_splits = std::max(0, cfg.small_splits);
  ov_.fp8_backward = cfg.fp8_backward;
  const StepPlan p = plan();
  ov_.small_path = p.small;  // the arena below is sized for these two
  ov_.fp8_backward = p.q8;
  const StepBufferBytes nb = step_buffer_bytes(p);

  const auto ft = symm_ ? build_sym_fwd_tiles(g_, sym_.jobs, sym_.nchunks) : build_fwd_tiles(g_);
  const auto dt = build_dz_tiles(g_);
  n_fwd_ = (int)ft.size();
  n_own_ = count_own_fwd_tiles(g_);
  n_dz_ = (int)dt.size();
  NTXENT_CHECK(n_fwd_ == (symm_ ? sym_.n_fwd : p.n_fwd) && n_own_ == p.n_own && n_dz_ == p.n_dz, "Engine: plan / tile list mismatch");
  ws_.bytes = gemm_workspace_bytes(std::max(n_fwd_, n_dz_), ws_.num_cus);

  struct Slot { void** p; size_t bytes; };
  // the symmetric mode (sym_step.h) keeps its own cosine / coefficient / slab layouts and sums
  // received contributions in launch_norm_bwd (no fused normalisation backward): its rows come
  // from the plan's SymBufferBytes (all 0 in the other modes)
  const SymBufferBytes& sb = sym_.bytes;
  const std::vector<Slot> slots = {
      {(void**)&zq_all_, nb.zq},
      {(void**)&zq8_all_, nb.zq8},
      {(void**)&zqt_all_, nb.zqt},
      {(void**)&zq8t_, nb.zq8t},
      {(void**)&q8_mneg_, nb.q8_mneg},
      {(void**)&q8_lmin_, nb.q8_lmin},
      {(void**)&inv_, nb.inv},
      {(void**)&ypos_, nb.ypos},
      {(void**)&part_, nb.part},
      {(void**)&sbuf_, symm_ ? sb.sbuf : nb.sbuf},
      {(void**)&cbuf_, symm_ ? sb.cbuf : nb.cbuf},
      {(void**)&lse2_all_, nb.lse2},
      {(void**)&cpos_, nb.cpos},
      {(void**)&block_loss_, nb.block_loss},
      {(void**)&loss_, nb.loss},
      {(void**)&one_, 4},
      {(void**)&slabs_, symm_ ? sb.own : nb.slabs},
      {(void**)&fold_pre_, nb.fold_pre},
      {(void**)&fold_cnt_, nb.fold_cnt},
      {(void**)&part_x_, sb.part_x},
      {(void**)&xsend_, sb.xsend},
      {(void**)&xrecv_, sb.xrecv},
      {(void**)&mbuf_, sb.mbuf},
      {(void**)&contrib_, sb.contrib},
      {(void**)&recv_, sb.recv},
      {(void**)&dz_rows_, sb.dz_rows},
      {(void**)&dotp_, symm_ ? 0 : nb.dotp},
      {(void**)&dot_, symm_ ? 0 : nb.dot},
      {(void**)&dot_cnt_, symm_ ? 0 : nb.dot_cnt},
      {(void**)&dtau_, nb.dtau},
      {(void**)&fwd_tiles_, ft.size() * sizeof(int4)},
      {(void**)&dz_tiles_, dt.size() * sizeof(int4)},
      {&ws_.ptr, ws_.bytes},
      {&small_scratch_, nb.small_scratch},
  };
  size_t total = 0;
  for (const auto& s : slots) total += align_up(s.bytes);
  arena_bytes_ = total;
  NTXENT_HIP_CHECK(hipMalloc(&arena_, total));
  char* base = static_cast<char*>(arena_);
  for (const auto& s : slots) {
    *s.p = s.bytes ? base : nullptr;
    base += align_up(s.bytes);
  }
  // zero once: the stream-K and LSE arrival counters are self-cleaning afterwards
  NTXENT_HIP_CHECK(hipMemset(arena_, 0, total));
  NTXENT_HIP_CHECK(hipMemcpy(fwd_tiles_, ft.data(), ft.size() * sizeof(int4), hipMemcpyHostToDevice));
  NTXENT_HIP_CHECK(hipMemcpy(dz_tiles_, dt.data(), dt.size() * sizeof(int4), hipMemcpyHostToDevice));
  if (sb.dz_rows) NTXENT_HIP_CHECK(hipMemcpy(dz_rows_, sym_.dz_rows.data(), sb.dz_rows, hipMemcpyHostToDevice));
  const float one = 1.0f;
  NTXENT_HIP_CHECK(hipMemcpy(one_, &one, 4, hipMemcpyHostToDevice));
  if (world_ > 1) {
    int lo = 0, hi = 0;
    NTXENT_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    NTXENT_HIP_CHECK(hipStreamCreateWithPriority(&comm_stream_, hipStreamNonBlocking, hi));
    NTXENT_HIP_CHECK(hipEventCreateWithFlags(&ev_prep_, hipEventDisableTiming));
    NTXENT_HIP_CHECK(hipEventCreateWithFlags(&ev_zq_, hipEventDisableTiming));
    NTXENT_HIP_CHECK(hipEventCreateWithFlags(&ev_zqt_, hipEventDisableTiming));
  }
  if (symm_) init_sym();
}

Engine::~Engine() {
  for (hipEvent_t e : ev_chunk_) hipEventDestroy(e);
  for (hipEvent_t e : {ev_f16_, ev_x_, ev_xdone_, ev_c_, ev_cdone_})
    if (e) hipEventDestroy(e);
  if (exec_) hipGraphExecDestroy(exec_);
  if (graph_) hipGraphDestroy(graph_);
  if (ev_prep_) hipEventDestroy(ev_prep_);
  if (ev_zq_) hipEventDestroy(ev_zq_);
  if (ev_zqt_) hipEventDestroy(ev_zqt_);
  if (comm_stream_) hipStreamDestroy(comm_stream_);
  if (rank_buf_) hipFree(rank_buf_);
  if (arena_) hipFree(arena_);
}

StepBuffers Engine::buffers(const float* grad_out, void* dh) const {
  StepBuffers b;
  b.h = h_;
  b.zq = zq_all_;
  b.zq8 = zq8_all_;
  b.zqt = zqt_all_;
  b.zq8t = zq8t_;
  b.inv = inv_;
  b.ypos = ypos_;
  b.part = part_;
  b.sbuf = sbuf_;
  b.cbuf = cbuf_;
  b.lse2 = lse2_all_;
  b.cpos = cpos_;
  b.q8_mneg = q8_mneg_;
  b.q8_lmin = q8_lmin_;
  b.block_loss = block_loss_;
  b.loss = loss_;
  b.fold_pre = fold_pre_;
  b.fold_cnt = fold_cnt_;
  b.dotp = dotp_;
  b.dot = dot_;
  b.dot_cnt = dot_cnt_;
  b.dtau = dtau_;
  b.slabs = slabs_;
  b.fwd_tiles = fwd_tiles_;
  b.dz_tiles = dz_tiles_;
  b.small_scratch = small_scratch_;
  b.grad_out = grad_out ? grad_out : one_;
  b.dh = dh;
  b.ws = ws_;
  return b;
}

GemmWorkspace Engine::ws_overlap() const {
  GemmWorkspace ws = ws_;
  ws.sched_cus = std::max(1, ws_.num_cus - std::min(cfg_.comm_reserve_cus, ws_.num_cus / 2));
  return ws;
}

void Engine::forward(const void* h, hipStream_t s) {
  NTXENT_TRACE("ntxent.forward");
  h_ = h;
  if (symm_) {
    forward_sym(s);
    return;
  }
  StepBuffers b = buffers(nullptr, nullptr);
  // both forward launches overlap a gather (rows, then ZqT): leave CUs for the RCCL kernels
  if (world_ > 1) b.ws = ws_overlap();
  step_forward(plan(), b, s, world_ > 1 ? this : nullptr);
}

void Engine::backward(const float* grad_out, void* dh, hipStream_t s) {
  NTXENT_TRACE("ntxent.backward");
  NTXENT_CHECK(h_ != nullptr, "backward() before forward()");
  if (symm_) {
    backward_sym(grad_out, dh, s);
    return;
  }
  step_backward(plan(), buffers(grad_out, dh), s, world_ > 1 ? this : nullptr);
}

// Gathers on the comm stream; the own-rank tiles only need this rank's slot.
void Engine::after_prep(hipStream_t s) {
  char* op_all = f8_ ? zq8_all_ : zq_all_;
  const size_t op_bytes = f8_ ? (size_t)g_.rows_pad * g_.ld_k8 : (size_t)g_.rows_pad * g_.ld_k * cs_;
  const size_t zt_bytes = (size_t)g_.dim_n * g_.ld_t * cs_;
  NTXENT_HIP_CHECK(hipEventRecord(ev_prep_, s));
  NTXENT_HIP_CHECK(hipStreamWaitEvent(comm_stream_, ev_prep_, 0));
  comm_->all_gather(op_all + (size_t)rank_ * op_bytes, op_all, op_bytes, comm_stream_);
  NTXENT_HIP_CHECK(hipEventRecord(ev_zq_, comm_stream_));
  // the backward's B operand: the ZqT blocks
  comm_->all_gather(zqt_all_ + (size_t)rank_ * zt_bytes, zqt_all_, zt_bytes, comm_stream_);
  NTXENT_HIP_CHECK(hipEventRecord(ev_zqt_, comm_stream_));
  zqt_pending_ = true;
}

void Engine::before_remote(hipStream_t s) { NTXENT_HIP_CHECK(hipStreamWaitEvent(s, ev_zq_, 0)); }

void Engine::after_lse(hipStream_t s) {
  NTXENT_TRACE("ntxent.lse_gather");
  comm_->all_gather(lse2_all_ + (size_t)rank_ * g_.rows_pad, lse2_all_, (size_t)g_.rows_pad * 4, s);
  comm_->all_reduce_sum(loss_, 1, s);
}

void Engine::before_dz(hipStream_t s) {
  if (!zqt_pending_) return;
  NTXENT_HIP_CHECK(hipStreamWaitEvent(s, ev_zqt_, 0));
  zqt_pending_ = false;
}

void Engine::positive_rank(const void* d_h, int* d_rank, float* d_pos, float* d_hard, hipStream_t s) {
  NTXENT_TRACE("ntxent.positive_rank");
  // this rank's rows alone, at temperature 1 (the rank does not depend on it)
  const Geometry g = make_geometry(cfg_.rows, cfg_.dim, 1, 0, 1.0f);
  const size_t zq_bytes = align_up((size_t)g.rows_pad * g.ld_k * cs_), row_bytes = align_up((size_t)g.rows * 4);
  if (!rank_buf_) NTXENT_HIP_CHECK(hipMalloc(&rank_buf_, zq_bytes + 2 * row_bytes));
  char* base = static_cast<char*>(rank_buf_);
  float* inv = reinterpret_cast<float*>(base + zq_bytes);
  float* ypos = reinterpret_cast<float*>(base + zq_bytes + row_bytes);
  launch_prep(cfg_.input, bwd_, d_h, base, inv, ypos, g, s);
  launch_pos_rank(bwd_, base, g, d_rank, d_pos, d_hard, s);
}

void Engine::set_temperature(float temperature) {
  NTXENT_CHECK(world_ == 1, "Engine::set_temperature: single-process engines only (world == 1)");
  NTXENT_CHECK(temperature > 0.f, "temperature must be positive");
  cfg_.temperature = temperature;
  g_.temperature = temperature;  // (as make_geometry)
  g_.inv_temp = 1.0f / temperature;
  if (exec_) { hipGraphExecDestroy(exec_); exec_ = nullptr; }
  if (graph_) { hipGraphDestroy(graph_); graph_ = nullptr; }
}

float Engine::temperature_grad(hipStream_t s) {
  NTXENT_CHECK(dtau_ != nullptr, "Engine::temperature_grad: EngineConfig::temperature_grad is off");
  float d = 0.f;
  NTXENT_HIP_CHECK(hipMemcpyAsync(&d, dtau_, 4, hipMemcpyDeviceToHost, s));
  NTXENT_HIP_CHECK(hipStreamSynchronize(s));
  return d;
}

void Engine::capture(const void* h, void* dh, hipStream_t s) {
  NTXENT_TRACE("ntxent.graph.capture");
  fault_point("graph");
  NTXENT_CHECK(s != nullptr, "graph capture needs a non-default stream");
  if (exec_) { hipGraphExecDestroy(exec_); exec_ = nullptr; }
  if (graph_) { hipGraphDestroy(graph_); graph_ = nullptr; }
  NTXENT_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  try {
    step(h, dh, s);
  } catch (...) {
    hipGraph_t g = nullptr;
    hipStreamEndCapture(s, &g);
    if (g) hipGraphDestroy(g);
    throw;
  }
  NTXENT_HIP_CHECK(hipStreamEndCapture(s, &graph_));
  NTXENT_HIP_CHECK(hipGraphInstantiate(&exec_, graph_, nullptr, nullptr, 0));
}

void Engine::replay(hipStream_t s) {
  NTXENT_CHECK(exec_ != nullptr, "replay() before capture()");
  NTXENT_HIP_CHECK(hipGraphLaunch(exec_, s));
}

float Engine::loss(hipStream_t s) {
  float l = 0.f;
  NTXENT_HIP_CHECK(hipMemcpyAsync(&l, loss_, 4, hipMemcpyDeviceToHost, s));
  NTXENT_HIP_CHECK(hipStreamSynchronize(s));
  if (comm_) comm_->check();
  if (cfg_.check_finite && !std::isfinite(l)) throw std::runtime_error("ntxent: non-finite loss");
  return l;
}

}  // namespace ntxent
