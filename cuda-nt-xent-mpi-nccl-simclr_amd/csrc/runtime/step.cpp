// The one-GPU step (see include/ntxent/step.h): decisions, buffer sizes and the launch sequence
// shared by the autograd op and the native Engine.
#include "ntxent/step.h"

#include <algorithm>

#include "ntxent/trace.h"

namespace ntxent {

StepPlan resolve_step_plan(const Geometry& g, DType in, DType comp, bool keep_cos, int num_cus,
                           const StepOverrides& ov) {
  StepPlan p;
  p.g = g;
  p.in = in;
  p.comp = comp;
  p.bwd = backward_dtype(comp);
  p.keep_cos = keep_cos;
  p.num_cus = num_cus;
  p.f8 = comp == DType::FP8;
  p.n_own = count_own_fwd_tiles(g);
  p.n_fwd = p.n_own + g.row_tiles * (g.col_tiles - g.row_tiles);
  p.n_dz = g.row_tiles * (g.dim_n / kTile);
  p.fwd_mfma = comp;
  p.bwd_mfma = p.bwd;
  p.small = (ov.small_path < 0 ? small_path_enabled() : ov.small_path != 0) && small_path_eligible(g, comp);
  if (p.small) {
    p.small_fwd_fused = small_fwd_fused(g);
    const int o = ov.small_splits < 0 ? small_splits_override() : ov.small_splits;
    p.small_splits = o > 0 ? std::min(o, small_rows_pad(g) / 64) : small_bwd_splits(g);
    return p;
  }
  p.q8 = keep_cos && fp8_backward_eligible(g, comp) &&
         (ov.fp8_backward < 0 ? fp8_backward_enabled() : ov.fp8_backward != 0);
  p.raw = keep_cos && !p.f8 && raw_forward_enabled() && raw_forward_eligible(g, in, comp);
  // (not on fp8 plans: dot_i = sum_j C_ij cos_ij would use the e4m3 forward's cosines, ~1e-2 off)
  p.fuse = !p.f8 && p.bwd != DType::F32 && g.dim % 8 == 0;
  GemmWorkspace ws;  // the backward's GEMMs overlap no transfer: the whole chip (sched_cus 0)
  ws.num_cus = num_cus;
  p.half_c = keep_cos && !p.q8 && half_c_enabled() && dz_half_c_eligible(p.bwd, g, p.n_dz, ws);
  p.dfold = p.fuse && !p.q8 && dz_dot_fold_eligible(p.bwd, g, p.n_dz, ws);
  // raw operands: the input rows themselves feed the forward MFMA
  p.fwd_mfma = p.raw ? in : comp;
  p.bwd_mfma = p.q8 ? DType::FP8 : p.bwd;
  return p;
}

StepBufferBytes step_buffer_bytes(const StepPlan& p) {
  const Geometry& g = p.g;
  const size_t W = g.world, Rp = g.rows_pad, R = g.rows, cs = dtype_size(p.bwd);
  StepBufferBytes n;
  n.zq = W * Rp * g.ld_k * cs;
  n.inv = n.ypos = R * 4;
  if (p.tau_grad) {  // every plan then has the per-row dot (the unfused paths store it as well)
    n.dot = Rp * 4;
    n.dtau = 4;
  }
  if (p.small) {
    n.lse2 = n.cpos = (size_t)small_rows_pad(g) * 4;
    n.small_scratch = small_scratch_bytes(g, std::max(small_bwd_splits(g), p.small_splits));
    return n;
  }
  n.zq8 = p.f8 ? W * Rp * g.ld_k8 : 0;
  n.zqt = p.q8 ? 0 : W * g.dim_n * g.ld_t * cs;
  n.zq8t = p.q8 ? (size_t)g.dim_n * q8_ldt(g) : 0;
  n.q8_mneg = p.q8 ? Rp * 4 : 0;
  n.q8_lmin = p.q8 ? 4 : 0;
  n.part = (size_t)g.col_tiles * Rp * sizeof(float2);
  n.sbuf = p.keep_cos ? (size_t)p.n_fwd * kTileElems * cs : 0;
  n.cbuf = (size_t)g.row_tiles * g.col_tiles * kTileElems * (p.q8 ? 1 : cs);
  n.lse2 = W * Rp * 4;
  n.cpos = Rp * 4;
  n.block_loss = (size_t)lse_scratch_floats(g) * 4;
  n.fold_pre = g.world == 1 ? Rp * sizeof(float2) : 0;
  n.fold_cnt = g.world == 1 ? (Rp / 64 + 1) * sizeof(int) : 0;
  n.dotp = p.fuse ? Rp * (size_t)dot_slots(g) * 4 : 0;
  n.dot = p.fuse || p.tau_grad ? Rp * 4 : 0;
  n.dot_cnt = p.fuse ? 2 * sizeof(int) : 0;
  n.slabs = Rp * g.dim_n * (p.bwd != DType::F32 ? 2 : 4);
  n.ws = gemm_workspace_bytes(std::max(p.n_fwd, p.n_dz), p.num_cus);
  return n;
}

namespace {
// this rank's slot of a gathered buffer (world 1: the buffer itself)
char* slot(void* base, size_t bytes_per_rank, const Geometry& g) {
  return base ? static_cast<char*>(base) + (size_t)g.rank * bytes_per_rank : nullptr;
}
}  // namespace

void step_forward(const StepPlan& p, const StepBuffers& b, hipStream_t s, StepComm* comm) {
  const Geometry& g = p.g;
  if (p.small) {  // one launch (row prologue fused up to kSmallFuseMaxRows): tiles + LSE merge + loss
    NTXENT_TRACE("ntxent.prep");
    fault_point("prep");
    if (!p.small_fwd_fused) launch_prep(p.in, p.bwd, b.h, b.zq, b.inv, b.ypos, g, s);
    NTXENT_TRACE("ntxent.small_fwd");
    fault_point("fwd");
    launch_small_fwd(p.in, p.comp, b.h, b.zq, b.inv, p.small_fwd_fused ? nullptr : b.ypos, b.lse2, b.cpos, b.loss,
                     b.small_scratch, g, s);
    if (fault_armed("nonfinite")) NTXENT_HIP_CHECK(hipMemsetAsync(b.loss, 0xFF, 4, s));  // NaN
    return;
  }
  NTXENT_CHECK(p.keep_cos || !p.f8, "step_forward: fp8 plans keep their cosines");
  const size_t Rp = g.rows_pad, cs = dtype_size(p.bwd);
  char* zq_local = slot(b.zq, Rp * g.ld_k * cs, g);
  char* zqt_local = slot(b.zqt, (size_t)g.dim_n * g.ld_t * cs, g);
  RawRows rr;  // raw-operand forward: no unit rows at all, the prologue computes inv and ypos only
  rr.h = b.h;
  rr.in = p.in;
  rr.inv = b.inv;
  rr.zqt = zqt_local;
  rr.zt = p.bwd;
  // the LSE launch's outputs: the diagonal remainder's launch may compute them (rr.lse_folded)
  rr.ypos = b.ypos;
  rr.lse2 = b.lse2;
  rr.cpos = b.cpos;
  rr.block_loss = b.block_loss;
  rr.loss = b.loss;
  rr.fold_pre = b.fold_pre;
  rr.fold_cnt = b.fold_cnt;
  // forward GEMM operand: the e4m3 rows for fp8 plans, else zq itself (raw: the input rows)
  char* zq8_local = slot(b.zq8, Rp * g.ld_k8, g);
  const void* op_all = p.raw ? nullptr : p.f8 ? b.zq8 : b.zq;
  const void* op_local = p.raw ? nullptr : p.f8 ? zq8_local : zq_local;
  {
    NTXENT_TRACE("ntxent.prep");
    fault_point("prep");
    launch_prep(p.in, p.bwd, b.h, p.raw ? nullptr : zq_local, b.inv, b.ypos, g, s, p.f8 ? zq8_local : nullptr);
    // one process: the transpose is written by the forward or the LSE launch (beside the merge)
    if (comm) launch_transpose(p.bwd, zq_local, zqt_local, g, s);
  }
  if (comm) comm->after_prep(s);
  bool zt_fwd = false;  // Z^T written by the forward launch (raw, beside the diagonal remainder)
  {
    NTXENT_TRACE("ntxent.fwd_gemm.own");
    fault_point("fwd");
    zt_fwd = launch_fwd_stats(p.comp, op_local, op_all, b.fwd_tiles, p.n_own, b.part, b.sbuf, b.ws, g, s, BlockView{},
                              nullptr, own_diag_tail(g), nullptr, p.raw ? &rr : nullptr);
  }
  if (p.n_fwd > p.n_own) {
    NTXENT_TRACE("ntxent.fwd_gemm.remote");
    if (comm) comm->before_remote(s);
    launch_fwd_stats(p.comp, op_local, op_all, b.fwd_tiles + p.n_own, p.n_fwd - p.n_own, b.part,
                     b.sbuf ? static_cast<char*>(b.sbuf) + (size_t)p.n_own * kTileElems * cs : nullptr, b.ws, g, s);
  }
  fault_point("lse");
  if (!rr.lse_folded) {
    NTXENT_TRACE("ntxent.lse");
    if (p.q8) {
      Q8Stats q8;
      q8.mneg2 = b.q8_mneg;
      q8.lmin = b.q8_lmin;
      q8.zq8t = b.zq8t;
      launch_lse(b.part, b.ypos, b.lse2, b.cpos, b.block_loss, b.loss, g, s, p.bwd, zq_local, nullptr, &q8);
    } else if (!comm) {
      launch_lse(b.part, b.ypos, b.lse2, b.cpos, b.block_loss, b.loss, g, s, p.bwd, p.raw ? nullptr : zq_local,
                 zt_fwd ? nullptr : zqt_local, nullptr, p.raw && !zt_fwd ? &rr : nullptr, rr.lse_fold_order);
    } else {
      launch_lse(b.part, b.ypos, b.lse2, b.cpos, b.block_loss, b.loss, g, s);
    }
  }
  if (comm) comm->after_lse(s);
  if (fault_armed("nonfinite")) NTXENT_HIP_CHECK(hipMemsetAsync(b.loss, 0xFF, 4, s));  // NaN
}

namespace {
// dL/dtau from the per-row dot the backward has just left in b.dot: the step's last launch
void tau_grad(const StepBuffers& b, const Geometry& g, hipStream_t s) {
  NTXENT_TRACE("ntxent.tau_grad");
  launch_tau_grad(b.dot, b.grad_out, b.dtau, g, s);
}
}  // namespace

void step_backward(const StepPlan& p, const StepBuffers& b, hipStream_t s, StepComm* comm) {
  const Geometry& g = p.g;
  NTXENT_CHECK(!p.tau_grad || (g.world == 1 && comm == nullptr && b.dot && b.dtau),
               "step_backward: the temperature gradient needs one rank and the dot / dtau buffers");
  float* dot_out = p.tau_grad ? b.dot : nullptr;  // the unfused paths store their per-row dot
  if (p.small) {
    NTXENT_TRACE("ntxent.small_bwd");
    fault_point("dz");
    launch_small_bwd(p.in, p.comp, b.zq, b.h, b.inv, b.lse2, b.cpos, b.grad_out, b.dh, b.small_scratch, g, s,
                     p.small_splits, dot_out);
    if (p.tau_grad) tau_grad(b, g, s);
    return;
  }
  const char* zq_local = slot(b.zq, (size_t)g.rows_pad * g.ld_k * dtype_size(p.bwd), g);
  Q8Stats q8;  // fp8 backward
  q8.mneg2 = b.q8_mneg;
  q8.lmin = b.q8_lmin;
  q8.zq = zq_local;
  float* dotp = p.fuse ? b.dotp : nullptr;
  {
    NTXENT_TRACE("ntxent.coef");
    fault_point("coef");
    if (p.keep_cos)  // half C: upper coefficient tiles only, the dZ reads the lower ones transposed
      launch_coef(p.bwd, b.sbuf, b.cbuf, b.lse2, b.cpos, b.fwd_tiles, p.n_fwd, g, s, nullptr, dotp,
                  p.q8 ? &q8 : nullptr, p.half_c);
    else  // recompute the cosines from the unit rows (their dtype: fp16 on an fp8 plan)
      launch_coef_gemm(p.bwd, zq_local, b.zq, b.cbuf, b.lse2, b.cpos, b.fwd_tiles, p.n_fwd, b.ws, g, s, BlockView{},
                       dotp);
    if (p.fuse && !p.dfold) launch_dot_reduce(b.dotp, b.dot, g, s);
  }
  if (comm) comm->before_dz(s);
  {
    NTXENT_TRACE("ntxent.dz_gemm");
    fault_point("dz");
    NormFuse nf;
    nf.h = b.h;
    nf.in = p.in;
    nf.inv = b.inv;
    nf.dot = b.dot;
    nf.grad_out = b.grad_out;
    nf.dh = b.dh;
    if (p.dfold) {  // the dot reduce folded into the dZ
      nf.dotp = b.dotp;
      nf.dot_cnt = b.dot_cnt;
    }
    const bool fused =
        p.q8 ? launch_dz(DType::FP8, b.cbuf, b.zq8t, b.dz_tiles, p.n_dz, b.slabs, b.ws, g, s, /*out_f16=*/true,
                         p.fuse ? &nf : nullptr, &q8, b.cpos)
             : launch_dz(p.bwd, b.cbuf, b.zqt, b.dz_tiles, p.n_dz, b.slabs, b.ws, g, s,
                         /*out_f16=*/p.bwd != DType::F32, p.fuse ? &nf : nullptr, nullptr, nullptr, p.half_c);
    if (fused) {  // dh written by the dZ epilogue; b.dot is complete once that launch has finished
      if (p.tau_grad) tau_grad(b, g, s);
      return;
    }
  }
  {
    NTXENT_TRACE("ntxent.norm_bwd");
    fault_point("norm_bwd");
    if (p.bwd != DType::F32)  // fp16 dZ slab (reduced-precision plans)
      launch_norm_bwd(p.in, nullptr, 0, b.h, b.inv, b.grad_out, b.dh, g, s, b.slabs, 1, dot_out);
    else
      launch_norm_bwd(p.in, static_cast<const float*>(b.slabs), 1, b.h, b.inv, b.grad_out, b.dh, g, s, nullptr, 0,
                      dot_out);
  }
  if (p.tau_grad) tau_grad(b, g, s);
}

}  // namespace ntxent
