// ntxent-mi355x — the one-GPU step: its decisions, its buffers and its launch sequence, once.
//
// Both host paths run a world-1 step through this module: the autograd op (fused_forward /
// fused_backward in ntxent_torch.cpp, buffers from torch's allocator) and the native Engine
// (engine.cpp, buffers from its arena). A feature of the step is wired in here and nowhere else.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "ntxent/ntxent.h"

namespace ntxent {

// What a caller may force instead of the process-wide toggles (EngineConfig's fields).
// small_path / fp8_backward: -1 the process default (set_small_path / set_fp8_backward), 0 off,
// 1 on where eligible. small_splits: -1 the process default (set_small_splits), 0
// small_bwd_splits, n > 0 that many backward column splits.
struct StepOverrides {
  int small_path = -1;
  int small_splits = -1;
  int fp8_backward = -1;
};

// Every decision of one step of (Geometry, input dtype, compute dtype, keep_cos). The LSE fold
// is not among them: it is an outcome of the forward launch (RawRows::lse_folded).
struct StepPlan {
  Geometry g;
  DType in = DType::BF16;    // dtype of h / dh
  DType comp = DType::F16;   // the plan's compute dtype (FP8: e4m3 forward GEMM)
  DType bwd = DType::F16;    // dtype of zq / Z^T / kept cosines / coefficients (backward_dtype)
  // cosine tiles kept for the backward (else the coefficient GEMM recomputes them). fp8 plans keep
  // them: callers pass keep_cos = true for a forward; false on an fp8 plan is only the autograd
  // op's second backward, which recomputes from the fp16 rows.
  bool keep_cos = true;
  bool small = false;            // small-problem path (small_kernels.hip)
  bool small_fwd_fused = false;  // ... whose forward runs the row prologue itself
  int small_splits = 0;          // ... and its backward column splits
  bool f8 = false;               // fp8 forward GEMM on the e4m3 rows zq8
  bool q8 = false;               // fp8 backward (e4m3 C and Z^T, Q8Stats)
  bool raw = false;              // raw-operand forward (RawRows): no unit rows
  bool fuse = false;             // normalisation backward in the dZ epilogue (NormFuse)
  bool half_c = false;           // upper coefficient tiles only (dz_half_c_eligible)
  bool dfold = false;            // dot reduce folded into the dZ (NormFuse::dot_cnt)
  int n_fwd = 0, n_own = 0, n_dz = 0;  // tiles of build_fwd_tiles (own block first) / build_dz_tiles
  int num_cus = 256;
  DType fwd_mfma = DType::F16;   // MFMA operand dtype the forward / backward GEMMs run
  DType bwd_mfma = DType::F16;
  // The caller's request, not a decision (resolve_step_plan leaves it false and no other field
  // depends on it): the backward also writes dL/dtau to StepBuffers::dtau (launch_tau_grad, the
  // step's last launch). World 1 only.
  bool tau_grad = false;
};

// The only caller of the *_eligible functions and *_enabled toggles outside the launchers' own
// argument checks. Cheap host code: resolve per call, so a toggle flipped between two calls takes
// effect on the next one.
StepPlan resolve_step_plan(const Geometry& g, DType in, DType comp, bool keep_cos, int num_cus,
                           const StepOverrides& ov = StepOverrides{});

// Device pointers of one step. A buffer whose step_buffer_bytes entry is 0 for the plan may be
// null. The buffers marked (z) hold self-cleaning counters: zero before their first use, and
// never shared by two streams.
struct StepBuffers {
  const void* h = nullptr;       // [rows][dim] input rows
  void* zq = nullptr;            // unit rows [Rpad][ld_k] (bwd dtype)
  void* zq8 = nullptr;           // e4m3 rows [Rpad][ld_k8] (f8)
  void* zqt = nullptr;           // Z^T [dim_n][ld_t] (bwd dtype)
  void* zq8t = nullptr;          // e4m3 Z^T [dim_n][q8_ldt] (q8)
  float* inv = nullptr;          // [rows]
  float* ypos = nullptr;         // [rows]
  float2* part = nullptr;        // [col_tiles][Rpad]
  void* sbuf = nullptr;          // kept cosines [n_fwd] tiles (keep_cos)
  void* cbuf = nullptr;          // coefficients [row_tiles][col_tiles] tiles
  float* lse2 = nullptr;         // [Rpad], log2 units
  float* cpos = nullptr;         // [Rpad] (small path: a_i)
  float* q8_mneg = nullptr;      // Q8Stats::mneg2 [Rpad], lmin [1]
  float* q8_lmin = nullptr;
  float* block_loss = nullptr;   // (z) lse_scratch_floats
  float* loss = nullptr;         // [1]
  float2* fold_pre = nullptr;    // folded LSE scratch [Rpad] (raw)
  int* fold_cnt = nullptr;       // (z) [Rpad / 64 + 1] (raw)
  float* dotp = nullptr;         // dot partials [dot_slots][Rpad] (fuse)
  float* dot = nullptr;          // [Rpad] (fuse, or tau_grad on any plan)
  float* dtau = nullptr;         // [1] dL/dtau (tau_grad)
  int* dot_cnt = nullptr;        // (z) [2] (dfold)
  void* slabs = nullptr;         // dZ [Rpad][dim_n], fp16 (fp32 plans: fp32); unused when the dZ fuses
  const int4* fwd_tiles = nullptr;
  const int4* dz_tiles = nullptr;
  void* small_scratch = nullptr; // (z) small path
  const float* grad_out = nullptr;  // device fp32 scalar
  void* dh = nullptr;            // [rows][dim]
  GemmWorkspace ws;              // (z) one workspace serves every GEMM launch of the step
};

// Byte size of each buffer of StepBuffers for a plan (0: the plan does not use it). The sizes do
// not depend on the toggles resolved per call (raw, dfold, small_fwd_fused): the Engine's arena,
// sized once, serves every later call; the autograd op allocates per call and skips what its
// plan's step does not touch (zq after a raw forward, fold_* without one, ...).
struct StepBufferBytes {
  size_t zq = 0, zq8 = 0, zqt = 0, zq8t = 0, inv = 0, ypos = 0, part = 0, sbuf = 0, cbuf = 0, lse2 = 0, cpos = 0,
         q8_mneg = 0, q8_lmin = 0, block_loss = 0, loss = 4, fold_pre = 0, fold_cnt = 0, dotp = 0, dot = 0,
         dot_cnt = 0, slabs = 0, small_scratch = 0, ws = 0, dtau = 0;
};
StepBufferBytes step_buffer_bytes(const StepPlan& p);

// Communication of the Engine's all-gather mode (world > 1), run between the same launches;
// null at world 1.
struct StepComm {
  virtual ~StepComm() = default;
  virtual void after_prep(hipStream_t s) = 0;    // start the gathers of the rows and of Z^T
  virtual void before_remote(hipStream_t s) = 0; // the remote forward tiles wait for the rows
  virtual void after_lse(hipStream_t s) = 0;     // gather the LSE, reduce the loss
  virtual void before_dz(hipStream_t s) = 0;     // the dZ waits for Z^T
};

// The launch sequence of one step, asynchronous on `stream`: prep -> forward GEMM (with or
// without the diagonal remainder and the LSE fold) -> LSE; coefficient pass -> optional dot
// reduce -> dZ -> optional normalisation backward; or the two small-path launches. With
// StepPlan::tau_grad one more launch ends the backward (launch_tau_grad over b.dot).
// Multi-rank (comm != null): b.zq / zq8 / zqt / lse2 point at the gathered buffers (this rank's
// slot at g.rank) and ws.sched_cus caps the forward GEMMs that overlap a gather.
void step_forward(const StepPlan& p, const StepBuffers& b, hipStream_t stream, StepComm* comm = nullptr);
void step_backward(const StepPlan& p, const StepBuffers& b, hipStream_t stream, StepComm* comm = nullptr);

}  // namespace ntxent
