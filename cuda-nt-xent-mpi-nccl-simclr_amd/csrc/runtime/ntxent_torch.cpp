// PyTorch (ROCm) op layer + Python binding of the MI355X NT-Xent kernels.
//
// Replaces the reference's host launchers (src/ntxent_kernel.cu:138-239) and its pybind11
// bindings (src/binding_new.cpp:4-21): same Python names and kwargs (`forward`, `backward`,
// `check_tensor_core_support`), plus
//   * TORCH_LIBRARY registration under `ntxent_cuda` (what python/test.py:137 expects) and
//     under `ntxent`;
//   * stage-level ops (prep / fwd_stats / lse / coef / dz / norm_bwd) over a cached `Plan`
//     (geometry + XCD-ordered tile lists resident on the device), which the Python autograd
//     Function and the RCCL data-parallel path compose;
//   * the symmetric data-parallel step's plan and phases (sym_step.h) over a bundle of tensors.
//
// No host synchronisation anywhere in these ops: they only enqueue on the current HIP stream.
#include <torch/extension.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPCachingAllocatorMasqueradingAsCUDA.h>

#include <algorithm>
#include <map>
#include <memory>
#include <atomic>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "ntxent/engine.h"
#include "ntxent/ntxent.h"
#include "ntxent/step.h"
#include "ntxent/sym_step.h"
#include "../kernels/pair_mask.h"  // the pair rule the kernels inline (pair_* bindings below)

namespace ntxent {
namespace th {

DType to_dtype(at::ScalarType t) {
  switch (t) {
    case at::kFloat: return DType::F32;
    case at::kHalf: return DType::F16;
    case at::kBFloat16: return DType::BF16;
    default: NTXENT_CHECK(false, std::string("unsupported dtype ") + c10::toString(t));
  }
  return DType::F32;
}

at::ScalarType to_scalar(DType t) {
  return t == DType::F32 ? at::kFloat : (t == DType::F16 ? at::kHalf : (t == DType::BF16 ? at::kBFloat16 : at::kByte));
}

// Compute-dtype policy. Normalised rows live in [-1, 1], where fp16's 10-bit mantissa beats
// bf16's 7 bits at equal MFMA rate, so reduced precision means fp16 unless asked otherwise.
DType choose_compute(at::ScalarType in, bool use_mixed_precision, const std::string& override_) {
  if (override_ == "fp32" || override_ == "float32") return DType::F32;
  if (override_ == "fp16" || override_ == "float16") return DType::F16;
  if (override_ == "bf16" || override_ == "bfloat16") return DType::BF16;
  if (override_ == "fp8" || override_ == "float8") return DType::FP8;
  NTXENT_CHECK(override_.empty() || override_ == "auto", "compute_dtype must be auto|fp32|fp16|bf16|fp8");
  if (in == at::kFloat && !use_mixed_precision) return DType::F32;
  return DType::F16;
}

struct Plan {
  Geometry g;
  DType comp = DType::F16;
  int device = 0;
  at::Tensor fwd_tiles;  // int32 [n, 4] on device
  int n_fwd = 0;
  int n_own = 0;  // own-rank tiles at the head of fwd_tiles
  at::Tensor dz_tiles;
  int n_dz = 0;
  int num_cus = 256;
  bool small = false;  // single-rank small-problem path (kernels/small_kernels.hip)

  int rows() const { return g.rows; }
  int rows_pad() const { return g.rows_pad; }
  int dim() const { return g.dim; }
  int dim_k() const { return g.dim_k; }
  int ld_k() const { return g.ld_k; }
  int ld_t() const { return g.ld_t; }
  int dim_n() const { return g.dim_n; }
  int world() const { return g.world; }
  int rank() const { return g.rank; }
  int row_tiles() const { return g.row_tiles; }
  int col_tiles() const { return g.col_tiles; }
  double temperature() const { return g.temperature; }
  std::string compute_dtype() const { return dtype_name(comp); }
  DType bwd() const { return backward_dtype(comp); }                  // zq / sc / C / ZqT dtype
  long op_ld() const { return comp == DType::FP8 ? g.ld_k8 : g.ld_k; }  // forward operand row stride
  std::string backward_dtype_name() const { return dtype_name(bwd()); }
};

static at::Tensor upload_tiles(const std::vector<int4>& v, int device) {
  auto cpu = torch::empty({(long)v.size(), 4}, torch::dtype(torch::kInt32));
  std::memcpy(cpu.data_ptr<int>(), v.data(), v.size() * sizeof(int4));
  return cpu.to(torch::Device(torch::kCUDA, device), /*non_blocking=*/false);
}

// The device tile lists depend on the shape alone: plans that differ only in temperature or
// compute dtype share one upload (a temperature that moves every step would otherwise upload two
// lists per step with a blocking copy and keep every one of them).
namespace {
struct TileLists {
  at::Tensor fwd_tiles, dz_tiles;
  int n_fwd = 0, n_own = 0, n_dz = 0;
};
std::atomic<long> g_tile_uploads{0};  // tile_list_uploads(): what the tests count

// caller holds get_plan's lock
std::shared_ptr<const TileLists> tile_lists(const Geometry& g, int device) {
  static std::map<std::tuple<int, int, int, int, int>, std::shared_ptr<const TileLists>> cache;
  auto key = std::make_tuple(g.rows, g.dim, g.world, g.rank, device);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  auto t = std::make_shared<TileLists>();
  auto ft = build_fwd_tiles(g);
  t->n_fwd = (int)ft.size();
  t->n_own = count_own_fwd_tiles(g);
  t->fwd_tiles = upload_tiles(ft, device);
  auto dt = build_dz_tiles(g);
  t->n_dz = (int)dt.size();
  t->dz_tiles = upload_tiles(dt, device);
  g_tile_uploads.fetch_add(1);
  cache.emplace(key, t);
  return t;
}
constexpr size_t kMaxPlans = 64;  // per-temperature Plan objects kept (least recently used goes first)
}  // namespace

std::shared_ptr<Plan> get_plan(int rows, int dim, int world, int rank, double temperature,
                               const std::string& compute, int device) {
  static std::mutex mu;
  struct Entry {
    std::shared_ptr<Plan> plan;
    unsigned long long used = 0;
  };
  static std::map<std::tuple<int, int, int, int, float, int, int>, Entry> cache;
  static unsigned long long tick = 0;
  const DType comp = choose_compute(at::kFloat, compute != "fp32" && compute != "float32", compute);
  auto key = std::make_tuple(rows, dim, world, rank, (float)temperature, (int)comp, device);
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(key);
  if (it != cache.end()) {
    it->second.used = ++tick;
    return it->second.plan;
  }
  auto p = std::make_shared<Plan>();
  p->g = make_geometry(rows, dim, world, rank, (float)temperature);
  p->comp = comp;
  p->device = device;
  const DeviceInfo& di = device_info(device);
  p->num_cus = di.num_cus;
  const auto tl = tile_lists(p->g, device);
  p->n_fwd = tl->n_fwd;
  p->n_own = tl->n_own;
  p->fwd_tiles = tl->fwd_tiles;
  p->n_dz = tl->n_dz;
  p->dz_tiles = tl->dz_tiles;
  StepOverrides small_on;  // eligibility, whatever set_small_path says
  small_on.small_path = 1;
  p->small = resolve_step_plan(p->g, DType::F16, comp, true, p->num_cus, small_on).small;
  if (cache.size() >= kMaxPlans) {  // (a plan still in use stays alive through its shared_ptr)
    auto lru = cache.begin();
    for (auto c = cache.begin(); c != cache.end(); ++c)
      if (c->second.used < lru->second.used) lru = c;
    cache.erase(lru);
  }
  cache.emplace(key, Entry{p, ++tick});
  return p;
}

static hipStream_t cur_stream(const at::Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

static void check_input(const at::Tensor& h, const char* name) {
  NTXENT_CHECK(h.is_cuda(), std::string(name) + " must be a GPU (HIP) tensor");
  NTXENT_CHECK(h.is_contiguous(), std::string(name) + " must be contiguous");
}

// stacked views [2N, d]: 2-D with an even, non-zero row count
static void check_stacked(const at::Tensor& h, const std::string& name = "h") {
  NTXENT_CHECK(h.dim() == 2, name + " must be 2-D [2N, d]");
  NTXENT_CHECK(h.size(0) > 0 && h.size(0) % 2 == 0, name + " must hold an even number of rows (two stacked views)");
}

// this rank's input rows [rows, dim] of the plan's geometry
static void check_h(const at::Tensor& h, const Geometry& g) {
  check_input(h, "h");
  NTXENT_CHECK(h.dim() == 2 && h.size(0) == g.rows && h.size(1) == g.dim, "h shape does not match plan");
}

// prep's inv of those rows
static void check_inv(const at::Tensor& inv, const Geometry& g) {
  NTXENT_CHECK(inv.numel() == g.rows && inv.scalar_type() == at::kFloat, "inv must be float32 [rows] (prep's output)");
}

// the first element of the incoming gradient as a contiguous fp32 [1] tensor on its device
static at::Tensor grad_scalar(const at::Tensor& grad_out) {
  return grad_out.to(at::kFloat).reshape({-1}).narrow(0, 0, 1).contiguous();
}

static at::TensorOptions opts(const at::Tensor& like, at::ScalarType t) {
  return at::TensorOptions().dtype(t).device(like.device());
}

// Zero-initialised scratch for the kernels' self-cleaning arrival counters (stream-K tile
// arrivals, LSE and small-path last-block-done tickets) and their partials. Every launch returns
// its counters to zero, so a buffer is zeroed only when it is (re)allocated and no memset runs
// per launch. The cache is keyed by (device, slot, STREAM): launches sharing one buffer are then
// always stream-ordered, and losses evaluated concurrently on different streams never race on
// one ticket (a counter reset in the middle of another stream's launch would leave it non-zero
// and starve every later last-arriver). A grown buffer replaces the old one; the caching
// allocator keeps the old block alive until its stream is done.
static at::Tensor device_scratch(const at::Tensor& like, size_t bytes, int slot) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, hipStream_t>, at::Tensor> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto& t = cache[{(int)like.device().index(), slot, cur_stream(like)}];
  if (!t.defined() || (size_t)t.numel() < bytes) t = at::zeros({(long)bytes}, opts(like, at::kByte));
  return t;
}


// reserve_cus: CUs this launch leaves free for communication kernels that overlap it (a
// per-launch argument: parallel/commstats.py:comm_reserve_cus), at most half the chip.
static GemmWorkspace gemm_ws(const at::Tensor& like, int ntiles, const Plan& P, int reserve_cus = 0) {
  NTXENT_CHECK(reserve_cus >= 0, "reserve_cus must be >= 0");
  GemmWorkspace ws;
  ws.num_cus = P.num_cus;
  ws.sched_cus = std::max(1, P.num_cus - std::min(reserve_cus, P.num_cus / 2));
  ws.bytes = gemm_workspace_bytes(ntiles, P.num_cus);
  ws.ptr = device_scratch(like, ws.bytes, 0).data_ptr();
  return ws;
}

// ---- stage ops ----------------------------------------------------------------------
// `zq_out` (optional): write the normalised rows into this [rows_pad, ld_k] buffer — e.g. this
// rank's slot of the all-gather destination, so the gather runs in place.
// Returns {zq, inv, ypos, zq8}: zq in the backward dtype; zq8 (uint8 e4m3 rows [rows_pad, ld_k8])
// only for fp8 plans (undefined otherwise), written into `zq8_out` when given.
std::vector<at::Tensor> prep(const at::Tensor& h, const Plan& P, const c10::optional<at::Tensor>& zq_out,
                             const c10::optional<at::Tensor>& zq8_out) {
  check_h(h, P.g);
  const at::DeviceGuard guard(h.device());
  at::Tensor zq;
  if (zq_out.has_value() && zq_out->defined()) {
    zq = *zq_out;
    check_input(zq, "zq_out");
    NTXENT_CHECK(zq.numel() == (long)P.g.rows_pad * P.g.ld_k && zq.scalar_type() == to_scalar(P.bwd()),
                 "zq_out must be [rows_pad, ld_k] in the backward dtype");
  } else {
    zq = at::empty({P.g.rows_pad, P.g.ld_k}, opts(h, to_scalar(P.bwd())));
  }
  at::Tensor zq8;
  if (P.comp == DType::FP8) {
    if (zq8_out.has_value() && zq8_out->defined()) {
      zq8 = *zq8_out;
      check_input(zq8, "zq8_out");
      NTXENT_CHECK(zq8.numel() == (long)P.g.rows_pad * P.g.ld_k8 && zq8.scalar_type() == at::kByte,
                   "zq8_out must be uint8 [rows_pad, ld_k8]");
    } else {
      zq8 = at::empty({P.g.rows_pad, P.g.ld_k8}, opts(h, at::kByte));
    }
  }
  auto inv = at::empty({P.g.rows}, opts(h, at::kFloat));
  auto ypos = at::empty({P.g.rows}, opts(h, at::kFloat));
  launch_prep(to_dtype(h.scalar_type()), P.bwd(), h.data_ptr(), zq.data_ptr(), inv.data_ptr<float>(),
              ypos.data_ptr<float>(), P.g, cur_stream(h), zq8.defined() ? zq8.data_ptr() : nullptr);
  return {zq, inv, ypos, zq8};
}

// Contrastive metrics, stage level: zq = prep's unit rows of a world-1 plan (its temperature plays
// no part). Returns {rank int32 [R], pos_cos fp32 [R], hard_neg_cos fp32 [R]} (launch_pos_rank).
std::vector<at::Tensor> pos_rank(const at::Tensor& zq, const Plan& P) {
  check_input(zq, "zq");
  NTXENT_CHECK(P.g.world == 1, "pos_rank: one rank only (a plan with world == 1)");
  NTXENT_CHECK(zq.numel() == (long)P.g.rows_pad * P.g.ld_k && zq.scalar_type() == to_scalar(P.bwd()),
               "zq must be [rows_pad, ld_k] in the plan's backward dtype");
  const at::DeviceGuard guard(zq.device());
  auto rank = at::empty({P.g.rows}, opts(zq, at::kInt));
  auto pos = at::empty({P.g.rows}, opts(zq, at::kFloat));
  auto hard = at::empty({P.g.rows}, opts(zq, at::kFloat));
  launch_pos_rank(P.bwd(), zq.data_ptr(), P.g, rank.data_ptr<int>(), pos.data_ptr<float>(), hard.data_ptr<float>(),
                  cur_stream(zq));
  return {rank, pos, hard};
}

// Contrastive metrics of stacked views h = [h1; h2] on the current stream: the row prologue and
// pos_rank. The compute dtype resolves as choose_compute does; "fp8" computes in fp16 (the rank
// kernel has no fp8 operands).
std::vector<at::Tensor> positive_rank(const at::Tensor& h, const std::string& compute, bool use_mixed_precision) {
  check_input(h, "h");
  check_stacked(h);
  const at::DeviceGuard guard(h.device());
  const DType comp = backward_dtype(choose_compute(h.scalar_type(), use_mixed_precision, compute));
  auto P = get_plan((int)h.size(0), (int)h.size(1), 1, 0, 1.0, dtype_name(comp), h.device().index());
  const auto st = prep(h, *P, c10::nullopt, c10::nullopt);
  return pos_rank(st[0], *P);
}

// ---- cross-view InfoNCE (kernels/xview_kernels.hip) -----------------------------------------
// The CLIP-form loss of stacked views h = [h1; h2] on the current stream: the row prologue, the
// N x N tile GEMM with its LSE epilogue and the LSE merge. The compute dtype resolves as
// choose_compute does; "fp8" computes in fp16 (these kernels have no fp8 operands).
// Returns {loss, inv, lse2, cpos}: what xview_backward needs besides h (the unit rows are not
// kept: the backward runs the row prologue again, and releases them before its largest buffer).
static std::shared_ptr<Plan> xview_plan(const at::Tensor& h, double T, DType comp) {
  return get_plan((int)h.size(0), (int)h.size(1), 1, 0, T, dtype_name(comp), h.device().index());
}

std::vector<at::Tensor> xview_forward(const at::Tensor& h, double T, const std::string& compute) {
  check_input(h, "h");
  check_stacked(h);
  const at::DeviceGuard guard(h.device());
  const DType comp = backward_dtype(choose_compute(h.scalar_type(), false, compute));
  auto P = xview_plan(h, T, comp);
  const Geometry& g = P->g;
  const auto st = prep(h, *P, c10::nullopt, c10::nullopt);  // {zq, inv, ypos, -}
  auto scratch = at::empty({(long)((xview_fwd_scratch_bytes(g) + 7) / 8)}, opts(h, at::kDouble));
  auto lse2 = at::empty({g.rows_pad}, opts(h, at::kFloat));
  auto cpos = at::empty({g.rows_pad}, opts(h, at::kFloat));
  auto loss = at::empty({}, opts(h, at::kFloat));
  launch_xview_fwd(comp, st[0].data_ptr(), st[2].data_ptr<float>(), g, lse2.data_ptr<float>(), cpos.data_ptr<float>(),
                   loss.data_ptr<float>(), scratch.data_ptr(), cur_stream(h));
  return {loss, st[1], lse2, cpos};
}

// The forward's statistics: lse2_all [world * rows_pad] (one GPU: world 1) and cpos [rows_pad], and
// what a backward takes besides, inv [rows]. msg: a caller's own message for all of them.
static void check_xview_stats(const at::Tensor& lse2_all, const at::Tensor& cpos, const Geometry& g,
                              const char* msg = nullptr) {
  NTXENT_CHECK(lse2_all.numel() == (long)g.world * g.rows_pad && lse2_all.scalar_type() == at::kFloat,
               msg ? msg : "lse2_all must be float32 [world*rows_pad]");
  NTXENT_CHECK(cpos.numel() == g.rows_pad && cpos.scalar_type() == at::kFloat,
               msg ? msg : "cpos must be float32 [rows_pad]");
}
static void check_xview_saved(const at::Tensor& inv, const at::Tensor& lse2_all, const at::Tensor& cpos,
                              const Geometry& g, const char* msg) {
  NTXENT_CHECK(inv.numel() == g.rows && inv.scalar_type() == at::kFloat, msg);
  check_xview_stats(lse2_all, cpos, g, msg);
}

// The end of every backward (the callers release coef and zt before it: before dh exists): the
// grad_out / (2N tau) scaling and the normalisation backward of the slab; dot: also
// dot_i = z_i . (C z)_i, [rows].
static at::Tensor xview_backward_tail(const at::Tensor& h, const at::Tensor& inv, const at::Tensor& go,
                                      const at::Tensor& dz, const Geometry& g, hipStream_t stream,
                                      at::Tensor* dot = nullptr) {
  auto dh = at::empty_like(h);
  if (dot) *dot = at::empty({g.rows}, opts(h, at::kFloat));
  launch_norm_bwd(to_dtype(h.scalar_type()), dz.data_ptr<float>(), 1, h.data_ptr(), inv.data_ptr<float>(),
                  go.data_ptr<float>(), dh.data_ptr(), g, stream, nullptr, 0, dot ? dot->data_ptr<float>() : nullptr);
  return dh;
}

// 16-bit plans of the pairwise sigmoid loss: the pairs' cosines from the input rows in fp32
// (launch_xview_sigmoid_pos), [R/2]; undefined for fp32 plans. The forward and the backward form them
// from the same h and inv: the same bits.
static at::Tensor sigmoid_pos_cos(const at::Tensor& h, const at::Tensor& inv, DType comp, const Geometry& g) {
  if (comp == DType::F32) return at::Tensor();
  auto pos = at::empty({g.rows / 2}, opts(h, at::kFloat));
  launch_xview_sigmoid_pos(to_dtype(h.scalar_type()), h.data_ptr(), inv.data_ptr<float>(), g, pos.data_ptr<float>(),
                           cur_stream(h));
  return pos;
}

// The one-GPU backward of both losses, after the caller's checks: dh, and in *dtau (null: not wanted)
// dL/dtau times grad_out, a 0-d fp32 tensor. launch_coef(zq, coef, zt, pos_cos, stream): the loss's
// transposes and coefficient block. bias_part not null: the sigmoid loss. Its tiles' sums of C are
// allocated here, after zt, and the pairs' cosines (sigmoid_pos_cos; null otherwise) live as long as
// the unit rows.
template <class LaunchCoef>
static at::Tensor xview_backward_body(const at::Tensor& h, const at::Tensor& inv, const at::Tensor& go, const Plan& P,
                                      at::Tensor* bias_part, at::Tensor* dtau, LaunchCoef launch_coef) {
  const Geometry& g = P.g;
  const hipStream_t stream = cur_stream(h);
  // buffers live only as long as a stage needs them (stream-ordered reuse by the allocator): the
  // unit rows until the coefficients exist, coefficients and transposes until the slab exists
  auto coef = at::empty({(long)xview_coef_bytes(P.comp, g)}, opts(h, at::kByte));
  auto zt = at::empty({(long)xview_zt_bytes(P.comp, g)}, opts(h, at::kByte));
  if (bias_part) *bias_part = at::empty({(long)(xview_sigmoid_bias_part_bytes(g) / 4)}, opts(h, at::kFloat));
  {
    // The row prologue runs a second time (a seventh launch and a second read of h) so that zq need
    // not be saved across the step. REQUIREMENT on launch_prep: for the same h, plan and device it
    // must reproduce the forward's zq bit for bit (no atomics, no launch-dependent summation order),
    // because the saved lse2 / cpos were formed from the forward's zq and the coefficients
    // exp2(cos - lse2) are formed from this one; a prologue that is not repeatable would make G
    // inconsistent with its own normaliser. test_gpu_infonce.py::test_prep_is_bitwise_repeatable
    // holds it to that.
    const auto st = prep(h, P, c10::nullopt, c10::nullopt);
    const at::Tensor pos = bias_part ? sigmoid_pos_cos(h, inv, P.comp, g) : at::Tensor();
    launch_coef(st[0].data_ptr(), coef.data_ptr(), zt.data_ptr(), pos.defined() ? pos.data_ptr<float>() : nullptr, stream);
  }
  auto dz = at::empty({(long)(xview_dz_bytes(g) / 4)}, opts(h, at::kFloat));
  launch_xview_dz(P.comp, coef.data_ptr(), zt.data_ptr(), g, dz.data_ptr<float>(), stream);
  coef.reset();
  zt.reset();
  at::Tensor dot;
  auto dh = xview_backward_tail(h, inv, go, dz, g, stream, &dot);
  if (dtau) {
    *dtau = at::empty({}, opts(h, at::kFloat));
    launch_tau_grad(dot.data_ptr<float>(), go.data_ptr<float>(), dtau->data_ptr<float>(), g, stream);
  }
  return dh;
}

// dtau as xview_backward_body's. compute: the forward's.
static at::Tensor xview_backward_impl(const at::Tensor& h, const at::Tensor& inv, const at::Tensor& lse2,
                                      const at::Tensor& cpos, const at::Tensor& grad_out, double T,
                                      const std::string& compute, at::Tensor* dtau) {
  check_input(h, "h");
  const at::DeviceGuard guard(h.device());
  auto P = xview_plan(h, T, backward_dtype(choose_compute(h.scalar_type(), false, compute)));
  check_xview_saved(inv, lse2, cpos, P->g,
                    "xview_backward: inv [rows], lse2 / cpos [rows_pad] in float32 (xview_forward's outputs)");
  return xview_backward_body(h, inv, grad_scalar(grad_out), *P, nullptr, dtau,
                             [&](void* zq, void* coef, void* zt, const float*, hipStream_t stream) {
                               launch_xview_coef(P->comp, zq, lse2.data_ptr<float>(), cpos.data_ptr<float>(), P->g, coef,
                                                 zt, stream);
                             });
}

at::Tensor xview_backward(const at::Tensor& h, const at::Tensor& inv, const at::Tensor& lse2, const at::Tensor& cpos,
                          const at::Tensor& grad_out, double T, const std::string& compute) {
  return xview_backward_impl(h, inv, lse2, cpos, grad_out, T, compute, nullptr);
}

// xview_backward plus the temperature gradient: (dh, dtau); dh is bitwise xview_backward's.
std::tuple<at::Tensor, at::Tensor> xview_backward_tau(const at::Tensor& h, const at::Tensor& inv,
                                                      const at::Tensor& lse2, const at::Tensor& cpos,
                                                      const at::Tensor& grad_out, double T,
                                                      const std::string& compute) {
  at::Tensor dtau;
  auto dh = xview_backward_impl(h, inv, lse2, cpos, grad_out, T, compute, &dtau);
  return {dh, dtau};
}

// ---- pairwise sigmoid loss, the SigLIP form (kernels/xview_kernels.hip) ----------------------------
// Stacked views h = [h1; h2] on the current stream: the row prologue and the N x N tile GEMM with the
// softplus epilogue. The compute dtype resolves as for xview_forward ("fp8" computes in fp16).
// Returns {loss, inv}: nothing else needs saving (no normaliser; the backward runs the prologue again).
std::vector<at::Tensor> xview_sigmoid_forward(const at::Tensor& h, double T, double bias, const std::string& compute) {
  check_input(h, "h");
  check_stacked(h);
  const at::DeviceGuard guard(h.device());
  const DType comp = backward_dtype(choose_compute(h.scalar_type(), false, compute));
  auto P = xview_plan(h, T, comp);
  const Geometry& g = P->g;
  const auto st = prep(h, *P, c10::nullopt, c10::nullopt);  // {zq, inv, -, -}
  auto scratch = at::empty({(long)(xview_sigmoid_scratch_bytes(g) / 8)}, opts(h, at::kDouble));
  auto loss = at::empty({}, opts(h, at::kFloat));
  const at::Tensor pos = sigmoid_pos_cos(h, st[1], comp, g);
  launch_xview_sigmoid_fwd(comp, st[0].data_ptr(), g, (float)bias, loss.data_ptr<float>(), scratch.data_ptr(),
                           cur_stream(h), pos.defined() ? pos.data_ptr<float>() : nullptr);
  return {loss, st[1]};
}

// (dh, dtau, dbias), the last two times grad_out as 0-d fp32 tensors, undefined unless wanted; dh is
// bitwise the same with or without them.
std::tuple<at::Tensor, at::Tensor, at::Tensor> xview_sigmoid_backward(const at::Tensor& h, const at::Tensor& inv,
                                                                      const at::Tensor& grad_out, double T, double bias,
                                                                      const std::string& compute, bool want_tau,
                                                                      bool want_bias) {
  check_input(h, "h");
  check_stacked(h);
  const at::DeviceGuard guard(h.device());
  auto P = xview_plan(h, T, backward_dtype(choose_compute(h.scalar_type(), false, compute)));
  const Geometry& g = P->g;
  check_inv(inv, g);
  auto go = grad_scalar(grad_out);
  at::Tensor bias_part, dtau, dbias;
  auto dh = xview_backward_body(h, inv, go, *P, &bias_part, want_tau ? &dtau : nullptr,
                                [&](void* zq, void* coef, void* zt, const float* pos, hipStream_t stream) {
                                  launch_xview_sigmoid_coef(P->comp, zq, g, (float)bias, coef, zt,
                                                            bias_part.data_ptr<float>(), stream, pos);
                                });
  if (want_bias) {
    dbias = at::empty({}, opts(h, at::kFloat));
    launch_xview_sigmoid_bias_grad(bias_part.data_ptr<float>(), go.data_ptr<float>(), dbias.data_ptr<float>(), g,
                                   cur_stream(h));
  }
  return {dh, dtau, dbias};
}

// ---- distributed cross-view InfoNCE: stage ops (parallel/infonce.py and parallel/emulate.py call
// the same three) ----------------------------------------------------------------------------------
// P: this rank's plan (get_plan(R, d, W, r, ...), fp32 | fp16 | bf16); zq_all [W * Rpad, ld_k]: every
// rank's prep rows in its slot.
static void check_xview_dist(const at::Tensor& zq_all, const Plan& P) {
  check_input(zq_all, "zq_all");
  NTXENT_CHECK(P.comp != DType::FP8, "xview_dist: fp32 | fp16 | bf16 plans (these kernels have no fp8 operands)");
  NTXENT_CHECK(zq_all.numel() == (long)P.g.world * P.g.rows_pad * P.g.ld_k && zq_all.scalar_type() == to_scalar(P.comp),
               "zq_all must be [world*rows_pad, ld_k] in the plan's compute dtype");
}

// Forward tiles of both sides against the rank slots [q_lo, q_hi) except q_skip (-1: none) into
// part (float32 [xview_dist_part_slots, rows_pad, 2]) and ypos (float32 [>= rows / 2]). The own slot
// (q == rank) needs only this rank's rows, so its tiles can run while the others are gathered.
static void check_xview_part(const at::Tensor& part, const at::Tensor& ypos, const Plan& P) {
  check_input(part, "part");
  check_input(ypos, "ypos");
  NTXENT_CHECK(part.numel() * 4 == (long)xview_part_bytes(P.g) && part.scalar_type() == at::kFloat,
               "part must be float32 [world * n_pad / 128, rows_pad, 2]");
  NTXENT_CHECK(ypos.numel() >= P.g.rows / 2 && ypos.scalar_type() == at::kFloat, "ypos must be float32 [>= rows / 2]");
}

void xview_dist_fwd(const at::Tensor& zq_all, const Plan& P, at::Tensor& part, at::Tensor& ypos, int q_lo, int q_hi,
                    int q_skip) {
  check_xview_dist(zq_all, P);
  check_xview_part(part, ypos, P);
  const at::DeviceGuard guard(zq_all.device());
  launch_xview_dist_fwd(P.comp, zq_all.data_ptr(), P.g, q_lo, q_hi, q_skip,
                        reinterpret_cast<float2*>(part.data_ptr<float>()), ypos.data_ptr<float>(), cur_stream(zq_all));
}

// Merge: writes this rank's slot of lse2_all (float32 [world * rows_pad]) and cpos (float32
// [rows_pad]); returns this rank's share of the loss, a 0-d float64 tensor (a SUM over the ranks,
// rounded to float32 once, gives the loss).
at::Tensor xview_dist_lse(const at::Tensor& part, const at::Tensor& ypos, at::Tensor& lse2_all, at::Tensor& cpos,
                          const Plan& P) {
  check_xview_part(part, ypos, P);
  check_xview_stats(lse2_all, cpos, P.g);
  const at::DeviceGuard guard(part.device());
  auto scratch = at::empty({(long)(xview_lse_scratch_bytes(P.g) / 8)}, opts(part, at::kDouble));
  auto loss = at::empty({}, opts(part, at::kDouble));
  launch_xview_dist_lse(reinterpret_cast<const float2*>(part.data_ptr<float>()), ypos.data_ptr<float>(), P.g,
                        lse2_all.data_ptr<float>(), cpos.data_ptr<float>(), loss.data_ptr<double>(), scratch.data_ptr(),
                        cur_stream(part));
  return loss;
}

// The rank-local backward of both losses from the gathered rows, after the caller's checks: the
// slots' transposes, then per side the coefficient block (one buffer, 4 n_pad W n_pad bytes) and its
// dZ rows, then the normalisation backward with the global scale grad_out / (2N tau).
// launch_coef(side, coef, pos_cos, stream): one side's coefficient block. bias_part as in
// xview_backward_body (allocated after coef; the pairs' cosines live across the two sides); dot as
// xview_backward_tail's.
template <class LaunchCoef>
static at::Tensor xview_dist_backward_body(const at::Tensor& h, const at::Tensor& zq_all, const at::Tensor& inv,
                                           const at::Tensor& go, const Plan& P, at::Tensor* bias_part, at::Tensor* dot,
                                           LaunchCoef launch_coef) {
  const Geometry& g = P.g;
  const hipStream_t stream = cur_stream(h);
  auto zt = at::empty({(long)xview_zt_bytes(P.comp, g)}, opts(h, at::kByte));
  auto coef = at::empty({(long)xview_coef_bytes(P.comp, g)}, opts(h, at::kByte));
  if (bias_part) *bias_part = at::empty({(long)(xview_sigmoid_bias_part_bytes(g) / 4)}, opts(h, at::kFloat));
  auto dz = at::empty({(long)(xview_dz_bytes(g) / 4)}, opts(h, at::kFloat));
  launch_xview_dist_zt(P.comp, zq_all.data_ptr(), g, g.world, zt.data_ptr(), stream);
  {
    const at::Tensor pos = bias_part ? sigmoid_pos_cos(h, inv, P.comp, g) : at::Tensor();
    for (int side = 0; side < 2; ++side) {
      launch_coef(side, coef.data_ptr(), pos.defined() ? pos.data_ptr<float>() : nullptr, stream);
      launch_xview_dist_dz(P.comp, coef.data_ptr(), zt.data_ptr(), g, g.world, side, dz.data_ptr<float>(), false, stream);
    }
  }
  coef.reset();
  zt.reset();
  return xview_backward_tail(h, inv, go, dz, g, stream, dot);
}

at::Tensor xview_dist_backward(const at::Tensor& h, const at::Tensor& zq_all, const at::Tensor& inv,
                               const at::Tensor& lse2_all, const at::Tensor& cpos, const at::Tensor& grad_out,
                               const Plan& P) {
  check_h(h, P.g);
  check_xview_dist(zq_all, P);
  check_xview_saved(inv, lse2_all, cpos, P.g,
                    "xview_dist_backward: inv [rows], cpos [rows_pad], lse2_all [world*rows_pad] in float32");
  const at::DeviceGuard guard(h.device());
  return xview_dist_backward_body(h, zq_all, inv, grad_scalar(grad_out), P, nullptr, nullptr,
                                  [&](int side, void* coef, const float*, hipStream_t stream) {
                                    launch_xview_dist_coef(P.comp, zq_all.data_ptr(), lse2_all.data_ptr<float>(),
                                                           cpos.data_ptr<float>(), P.g, side, coef, stream);
                                  });
}

// ---- distributed pairwise sigmoid loss: stage ops (parallel/sigmoid.py and parallel/emulate.py call
// the same three) ----------------------------------------------------------------------------------
// Side 0's forward tiles against the rank slots [q_lo, q_hi) except q_skip (-1: none) into the
// caller's lpart (float64 [xview_sigmoid_dist_tiles]); every tile has its own place there. h, inv:
// this rank's rows and prep's inv: a 16-bit plan whose slots include the own one takes the positives'
// cosines from them (the own slot alone holds positives).
static void check_lpart(const at::Tensor& lpart, const Geometry& g) {
  check_input(lpart, "lpart");
  NTXENT_CHECK(lpart.numel() * 8 == (long)xview_sigmoid_scratch_bytes(g) && lpart.scalar_type() == at::kDouble,
               "lpart must be float64 [n_pad / 128 * world * n_pad / 128]");
}

void xview_sigmoid_dist_fwd(const at::Tensor& zq_all, const Plan& P, at::Tensor& lpart, const at::Tensor& h,
                            const at::Tensor& inv, double bias, int q_lo, int q_hi, int q_skip) {
  check_xview_dist(zq_all, P);
  const Geometry& g = P.g;
  check_lpart(lpart, g);
  check_h(h, g);
  check_inv(inv, g);
  const at::DeviceGuard guard(zq_all.device());
  const bool own = q_lo <= g.rank && g.rank < q_hi && q_skip != g.rank;
  const at::Tensor pos = own ? sigmoid_pos_cos(h, inv, P.comp, g) : at::Tensor();
  launch_xview_sigmoid_dist_fwd(P.comp, zq_all.data_ptr(), nullptr, g, (float)bias, q_lo, q_hi, q_skip,
                                lpart.data_ptr<double>(), cur_stream(zq_all),
                                pos.defined() ? pos.data_ptr<float>() : nullptr);
}

// This rank's share of the loss, a 0-d float64 tensor (a SUM over the ranks, rounded to float32 once,
// gives the loss).
at::Tensor xview_sigmoid_dist_loss(const at::Tensor& lpart, const Plan& P) {
  check_lpart(lpart, P.g);
  const at::DeviceGuard guard(lpart.device());
  auto share = at::empty({}, opts(lpart, at::kDouble));
  launch_xview_sigmoid_dist_loss(lpart.data_ptr<double>(), P.g, share.data_ptr<double>(), cur_stream(lpart));
  return share;
}

// This rank's fp64 shares of (dL/dtau, dL/dbias) times grad_out, float64 [2] (an entry not wanted is
// zero); undefined if neither is wanted. dot: xview_backward_tail's; bias_part: side 0's sums of C.
static at::Tensor sigmoid_scalar_shares(const at::Tensor& dot, const at::Tensor& bias_part, const at::Tensor& go,
                                        const Geometry& g, bool want_tau, bool want_bias, hipStream_t stream) {
  at::Tensor shares;
  if (want_tau || want_bias) {
    shares = at::zeros({2}, opts(dot, at::kDouble));
    if (want_tau)
      launch_tau_grad(dot.data_ptr<float>(), go.data_ptr<float>(), nullptr, g, stream, shares.data_ptr<double>());
    if (want_bias)
      launch_xview_sigmoid_bias_grad(bias_part.data_ptr<float>(), go.data_ptr<float>(), nullptr, g, stream,
                                     shares.data_ptr<double>() + 1);
  }
  return shares;
}

// Rank-local backward from the gathered rows (xview_dist_backward_body). Returns (dh, shares):
// sigmoid_scalar_shares'; dh is bitwise the same with or without them.
std::tuple<at::Tensor, at::Tensor> xview_sigmoid_dist_backward(const at::Tensor& h, const at::Tensor& zq_all,
                                                               const at::Tensor& inv, const at::Tensor& grad_out,
                                                               const Plan& P, double bias, bool want_tau,
                                                               bool want_bias) {
  check_h(h, P.g);
  check_xview_dist(zq_all, P);
  check_inv(inv, P.g);
  const at::DeviceGuard guard(h.device());
  auto go = grad_scalar(grad_out);
  at::Tensor bias_part, dot;
  auto dh = xview_dist_backward_body(
      h, zq_all, inv, go, P, &bias_part, &dot, [&](int side, void* coef, const float* pos, hipStream_t stream) {
        launch_xview_sigmoid_dist_coef(P.comp, zq_all.data_ptr(), nullptr, 0, P.g, (float)bias, side, coef,
                                       side == 0 ? bias_part.data_ptr<float>() : nullptr, stream, pos);
      });
  return {dh, sigmoid_scalar_shares(dot, bias_part, go, P.g, want_tau, want_bias, cur_stream(h))};
}

// ---- the same loss, one rank slot at a time (exchange="ring"): stage ops shared by
// parallel/sigmoid.py's RingSigmoidFunction and parallel/emulate.py -----------------------------------
// zq [rows_pad, ld_k]: this rank's own prep rows; rows_q: the same shape, rank q's rows (q == rank: zq).
// bias_part and the fp32 slab dz are the caller's from the first block to xview_sigmoid_ring_finish.
static void check_bias_part(const at::Tensor& bias_part, const Geometry& g) {
  check_input(bias_part, "bias_part");
  NTXENT_CHECK(bias_part.numel() * 4 == (long)xview_sigmoid_bias_part_bytes(g) && bias_part.scalar_type() == at::kFloat,
               "bias_part must be float32 [n_pad / 128 * world * n_pad / 128 * 4]");
}
static void check_dz_slab(const at::Tensor& dz, const Geometry& g) {
  check_input(dz, "dz");
  NTXENT_CHECK(dz.numel() * 4 == (long)xview_dz_bytes(g) && dz.scalar_type() == at::kFloat,
               "dz must be float32 [rows_pad * dim_n]");
}
static void check_xview_block(const at::Tensor& zq, const at::Tensor& rows_q, int q, const Plan& P) {
  check_input(zq, "zq");
  check_input(rows_q, "rows_q");
  NTXENT_CHECK(P.comp != DType::FP8, "xview_block: fp32 | fp16 | bf16 plans (these kernels have no fp8 operands)");
  const long want = (long)P.g.rows_pad * P.g.ld_k;
  NTXENT_CHECK(zq.numel() == want && zq.scalar_type() == to_scalar(P.comp) && rows_q.numel() == want &&
                   rows_q.scalar_type() == to_scalar(P.comp),
               "zq and rows_q must be [rows_pad, ld_k] in the plan's compute dtype (whole rank slots)");
  NTXENT_CHECK(0 <= q && q < P.g.world, "slot q outside the world");
}

// 16-bit plans: the pairs' cosines of this rank's rows (sigmoid_pos_cos), the own block's diagonal in
// the block backward; undefined (None) for fp32 plans.
c10::optional<at::Tensor> xview_sigmoid_pos_cos(const at::Tensor& h, const at::Tensor& inv, const Plan& P) {
  check_h(h, P.g);
  check_inv(inv, P.g);
  const at::DeviceGuard guard(h.device());
  const at::Tensor pos = sigmoid_pos_cos(h, inv, P.comp, P.g);
  if (!pos.defined()) return c10::nullopt;
  return pos;
}

// Side 0's nT x nT tiles of a_r against b_q into the caller's lpart (float64 [xview_sigmoid_dist_tiles]),
// each at the place the gather launch gives it: after all W blocks xview_sigmoid_dist_loss serves as
// it is. h, inv: a 16-bit plan's own block (q == rank) takes the positives' cosines from them.
void xview_sigmoid_block_fwd(const at::Tensor& zq, const at::Tensor& rows_q, int q, const Plan& P, at::Tensor& lpart,
                             const at::Tensor& h, const at::Tensor& inv, double bias) {
  check_xview_block(zq, rows_q, q, P);
  const Geometry& g = P.g;
  check_lpart(lpart, g);
  check_h(h, g);
  check_inv(inv, g);
  const at::DeviceGuard guard(zq.device());
  const at::Tensor pos = q == g.rank ? sigmoid_pos_cos(h, inv, P.comp, g) : at::Tensor();
  launch_xview_sigmoid_dist_fwd(P.comp, zq.data_ptr(), rows_q.data_ptr(), g, (float)bias, q, q + 1, -1,
                                lpart.data_ptr<double>(), cur_stream(zq), pos.defined() ? pos.data_ptr<float>() : nullptr);
}

// One block of the backward: rows_q transposed into zt, then for side 0 and side 1 the coefficient
// block into coef and its product added to (first: stored in) the fp32 slab dz. coef
// (xview_block_coef_bytes), zt (xview_block_zt_bytes), bias_part (xview_sigmoid_bias_part_bytes / 4
// floats) and dz (xview_dz_bytes / 4 floats) are the caller's and are reused across blocks; none
// needs initialisation. pos_cos: xview_sigmoid_pos_cos's (None for fp32 plans).
void xview_sigmoid_block_backward(const at::Tensor& zq, const at::Tensor& rows_q, int q, const Plan& P, double bias,
                                  at::Tensor& coef, at::Tensor& zt, at::Tensor& bias_part, at::Tensor& dz,
                                  const c10::optional<at::Tensor>& pos_cos, bool first) {
  check_xview_block(zq, rows_q, q, P);
  check_input(coef, "coef");
  check_input(zt, "zt");
  const Geometry& g = P.g;
  NTXENT_CHECK(coef.numel() * coef.element_size() == (long)xview_block_coef_bytes(P.comp, g),
               "coef must hold xview_block_coef_bytes");
  NTXENT_CHECK(zt.numel() * zt.element_size() == (long)xview_block_zt_bytes(P.comp, g),
               "zt must hold xview_block_zt_bytes");
  check_bias_part(bias_part, g);
  check_dz_slab(dz, g);
  const float* pos = nullptr;
  if (pos_cos.has_value() && pos_cos->defined()) {
    check_input(*pos_cos, "pos_cos");
    NTXENT_CHECK(pos_cos->numel() == g.rows / 2 && pos_cos->scalar_type() == at::kFloat, "pos_cos must be float32 [rows / 2]");
    pos = pos_cos->data_ptr<float>();
  }
  NTXENT_CHECK((pos != nullptr) == (P.comp != DType::F32), "pos_cos with 16-bit plans and only there");
  const at::DeviceGuard guard(zq.device());
  const hipStream_t stream = cur_stream(zq);
  launch_xview_dist_zt(P.comp, rows_q.data_ptr(), g, 1, zt.data_ptr(), stream);
  for (int side = 0; side < 2; ++side) {
    launch_xview_sigmoid_dist_coef(P.comp, zq.data_ptr(), rows_q.data_ptr(), q, g, (float)bias, side, coef.data_ptr(),
                                   side == 0 ? bias_part.data_ptr<float>() : nullptr, stream, pos);
    launch_xview_dist_dz(P.comp, coef.data_ptr(), zt.data_ptr(), g, 1, side, dz.data_ptr<float>(), !first, stream);
  }
}

// After all W blocks (the caller has released coef and zt): the normalisation backward of the slab with
// the global scale. Returns (dh, shares): sigmoid_scalar_shares', as xview_sigmoid_dist_backward.
std::tuple<at::Tensor, at::Tensor> xview_sigmoid_ring_finish(const at::Tensor& h, const at::Tensor& inv,
                                                             const at::Tensor& grad_out, const at::Tensor& dz,
                                                             const at::Tensor& bias_part, const Plan& P, bool want_tau,
                                                             bool want_bias) {
  const Geometry& g = P.g;
  check_h(h, g);
  check_inv(inv, g);
  check_dz_slab(dz, g);
  check_bias_part(bias_part, g);
  const at::DeviceGuard guard(h.device());
  const hipStream_t stream = cur_stream(h);
  auto go = grad_scalar(grad_out);
  at::Tensor dot;
  auto dh = xview_backward_tail(h, inv, go, dz, g, stream, &dot);
  return {dh, sigmoid_scalar_shares(dot, bias_part, go, g, want_tau, want_bias, stream)};
}

at::Tensor transpose(const at::Tensor& zq, const Plan& P, const c10::optional<at::Tensor>& zqt_out) {
  check_input(zq, "zq");
  const at::DeviceGuard guard(zq.device());
  at::Tensor zqt;
  if (zqt_out.has_value() && zqt_out->defined()) {
    zqt = *zqt_out;
    check_input(zqt, "zqt_out");
    NTXENT_CHECK(zqt.numel() == (long)P.g.dim_n * P.g.ld_t && zqt.scalar_type() == zq.scalar_type(),
                 "zqt_out must be [dim_n, ld_t]");
  } else {
    zqt = at::empty({P.g.dim_n, P.g.ld_t}, zq.options());
  }
  launch_transpose(P.bwd(), zq.data_ptr(), zqt.data_ptr(), P.g, cur_stream(zq));
  return zqt;
}

// zero_cos: the raw op (Python fwd_stats) returns zeros in the lower 64x64 regions of diagonal
// tiles, which the forward may leave unwritten (the coefficient pass mirrors them from the upper
// ones, diag_up_kernel); the training path keeps the buffer uninitialised (a 66 MiB memset per
// step at the headline otherwise)
std::vector<at::Tensor> fwd_stats(const at::Tensor& zq_local, const at::Tensor& zq_all, const Plan& P,
                                  bool keep_cos, bool zero_cos = false) {
  check_input(zq_local, "zq_local");
  check_input(zq_all, "zq_all");
  NTXENT_CHECK(zq_all.size(0) == (long)P.g.world * P.g.rows_pad && zq_all.size(1) == P.op_ld(),
               "zq_all must be [world*rows_pad, ld] in the forward operand dtype (ld_k, or ld_k8 for fp8)");
  const at::DeviceGuard guard(zq_local.device());
  auto part = at::empty({P.g.col_tiles, P.g.rows_pad, 2}, opts(zq_local, at::kFloat));
  at::Tensor sc;
  if (keep_cos)
    sc = zero_cos ? at::zeros({(long)P.n_fwd * kTileElems}, opts(zq_local, to_scalar(P.bwd())))
                  : at::empty({(long)P.n_fwd * kTileElems}, opts(zq_local, to_scalar(P.bwd())));
  auto ws = gemm_ws(zq_local, P.n_fwd, P);
  launch_fwd_stats(P.comp, zq_local.data_ptr(), zq_all.data_ptr(),
                   reinterpret_cast<const int4*>(P.fwd_tiles.data_ptr<int>()), P.n_fwd,
                   reinterpret_cast<float2*>(part.data_ptr<float>()), sc.defined() ? sc.data_ptr() : nullptr,
                   ws, P.g, cur_stream(zq_local), BlockView{}, nullptr,
                   P.n_fwd == P.n_own ? own_diag_tail(P.g) : 0);
  return {part, sc};
}

// Forward tiles [first, first + count) of the plan's list into caller-owned `part` / `sc`
// (sc may be undefined). The own-rank tiles come first (P.n_own of them) and read only this
// rank's slot of zq_all, so they can run while the rest of zq_all is being gathered.
void fwd_stats_range(const at::Tensor& zq_local, const at::Tensor& zq_all, const Plan& P, at::Tensor& part,
                     const c10::optional<at::Tensor>& sc, int first, int count, int reserve_cus) {
  check_input(zq_local, "zq_local");
  check_input(zq_all, "zq_all");
  check_input(part, "part");
  NTXENT_CHECK(first >= 0 && count >= 0 && first + count <= P.n_fwd, "tile range out of bounds");
  NTXENT_CHECK(part.numel() == (long)P.g.col_tiles * P.g.rows_pad * 2 && part.scalar_type() == at::kFloat,
               "part must be float32 [col_tiles, rows_pad, 2]");
  NTXENT_CHECK(zq_all.numel() == (long)P.g.world * P.g.rows_pad * P.op_ld(),
               "zq_all must be [world*rows_pad, ld] in the forward operand dtype");
  const bool keep = sc.has_value() && sc->defined();
  if (keep) NTXENT_CHECK(sc->numel() == (long)P.n_fwd * kTileElems, "sc must hold n_fwd tiles");
  if (count == 0) return;
  const at::DeviceGuard guard(zq_local.device());
  auto ws = gemm_ws(zq_local, count, P, reserve_cus);
  char* scp = keep ? static_cast<char*>(sc->data_ptr()) + (size_t)first * kTileElems * dtype_size(P.bwd()) : nullptr;
  launch_fwd_stats(P.comp, zq_local.data_ptr(), zq_all.data_ptr(),
                   reinterpret_cast<const int4*>(P.fwd_tiles.data_ptr<int>()) + first, count,
                   reinterpret_cast<float2*>(part.data_ptr<float>()), scp, ws, P.g, cur_stream(zq_local), BlockView{},
                   nullptr, first + count == P.n_own ? std::min(count, own_diag_tail(P.g)) : 0);
}

// Writes this rank's slice of lse2_all (log2 units) and cpos (the positive coefficient
// -(a_i + a_p) of the local rows); returns the local loss contribution.
at::Tensor lse(const at::Tensor& part, const at::Tensor& ypos, at::Tensor& lse2_all, at::Tensor& cpos,
               const Plan& P, const c10::optional<at::Tensor>& zq = c10::nullopt,
               const c10::optional<at::Tensor>& zqt = c10::nullopt) {
  check_input(part, "part");
  NTXENT_CHECK(lse2_all.numel() == (long)P.g.world * P.g.rows_pad && lse2_all.scalar_type() == at::kFloat,
               "lse2_all must be float32 [world*rows_pad]");
  NTXENT_CHECK(cpos.numel() >= P.g.rows_pad && cpos.scalar_type() == at::kFloat, "cpos must be float32 [>= rows_pad]");
  const at::DeviceGuard guard(part.device());
  auto block_loss = device_scratch(part, (size_t)lse_scratch_floats(P.g) * 4, 1);
  auto loss = at::empty({}, opts(part, at::kFloat));
  const bool tr = zq.has_value() && zq->defined();
  if (tr) {  // also write zqt = zq^T (the rank-local rows) from the same launch
    NTXENT_CHECK(zqt.has_value() && zqt->defined(), "lse: zqt missing");
    check_input(*zq, "zq");
    check_input(*zqt, "zqt");
    NTXENT_CHECK(zq->numel() == (long)P.g.rows_pad * P.g.ld_k && zq->scalar_type() == to_scalar(P.bwd()),
                 "lse: zq must be [rows_pad, ld_k] in the backward dtype");
    NTXENT_CHECK(zqt->numel() == (long)P.g.dim_n * P.g.ld_t && zqt->scalar_type() == zq->scalar_type(),
                 "lse: zqt must be [dim_n, ld_t]");
  }
  launch_lse(reinterpret_cast<const float2*>(part.data_ptr<float>()), ypos.data_ptr<float>(),
             lse2_all.data_ptr<float>(), cpos.data_ptr<float>(), static_cast<float*>(block_loss.data_ptr()),
             loss.data_ptr<float>(), P.g, cur_stream(part), P.bwd(), tr ? zq->data_ptr() : nullptr,
             tr ? zqt->data_ptr() : nullptr);
  return loss;
}

// Kept cosines (compact, one slot per forward tile) -> coefficient buffer (all tiles).
at::Tensor coef(const at::Tensor& sbuf, const at::Tensor& lse2_all, const at::Tensor& cpos, const Plan& P) {
  check_input(sbuf, "sbuf");
  NTXENT_CHECK(sbuf.numel() == (long)P.n_fwd * kTileElems, "sbuf does not match the plan's forward tiles");
  const at::DeviceGuard guard(sbuf.device());
  auto cbuf = at::empty({(long)P.g.row_tiles * P.g.col_tiles * kTileElems}, sbuf.options());
  launch_coef(P.bwd(), sbuf.data_ptr(), cbuf.data_ptr(), lse2_all.data_ptr<float>(), cpos.data_ptr<float>(),
              reinterpret_cast<const int4*>(P.fwd_tiles.data_ptr<int>()), P.n_fwd, P.g, cur_stream(sbuf));
  return cbuf;
}

at::Tensor coef_gemm(const at::Tensor& zq_local, const at::Tensor& zq_all, const at::Tensor& lse2_all,
                     const at::Tensor& cpos, const Plan& P) {
  check_input(zq_local, "zq_local");
  const at::DeviceGuard guard(zq_local.device());
  auto cbuf = at::empty({(long)P.g.row_tiles * P.g.col_tiles * kTileElems}, opts(zq_local, to_scalar(P.bwd())));
  auto ws = gemm_ws(zq_local, P.n_fwd, P);
  launch_coef_gemm(P.comp, zq_local.data_ptr(), zq_all.data_ptr(), cbuf.data_ptr(), lse2_all.data_ptr<float>(),
                   cpos.data_ptr<float>(), reinterpret_cast<const int4*>(P.fwd_tiles.data_ptr<int>()), P.n_fwd,
                   ws, P.g, cur_stream(zq_local));
  return cbuf;
}

at::Tensor dz(const at::Tensor& sc, const at::Tensor& zqt_all, const Plan& P) {
  check_input(sc, "sc");
  check_input(zqt_all, "zqt_all");
  NTXENT_CHECK(zqt_all.numel() == (long)P.g.world * P.g.dim_n * P.g.ld_t, "zqt_all must be [world, dim_n, ld_t]");
  const at::DeviceGuard guard(sc.device());
  // reduced-precision plans keep dZ in fp16 (half the store and the normalisation backward's read)
  const bool f16 = P.bwd() != DType::F32;
  auto slabs = at::empty({1, P.g.rows_pad, P.g.dim_n}, opts(sc, f16 ? at::kHalf : at::kFloat));
  auto ws = gemm_ws(sc, P.n_dz, P);
  launch_dz(P.bwd(), sc.data_ptr(), zqt_all.data_ptr(), reinterpret_cast<const int4*>(P.dz_tiles.data_ptr<int>()),
            P.n_dz, slabs.data_ptr(), ws, P.g, cur_stream(sc), f16);
  return slabs;
}

at::Tensor norm_bwd(const at::Tensor& slabs, const at::Tensor& h, const at::Tensor& inv, const at::Tensor& grad_out,
                    const Plan& P) {
  check_input(h, "h");
  const at::DeviceGuard guard(h.device());
  auto go = grad_out.to(at::kFloat).contiguous();
  auto dh = at::empty_like(h);
  if (slabs.scalar_type() == at::kHalf)  // one fp16 dZ slab (dz() of a reduced-precision plan)
    launch_norm_bwd(to_dtype(h.scalar_type()), nullptr, 0, h.data_ptr(), inv.data_ptr<float>(), go.data_ptr<float>(),
                    dh.data_ptr(), P.g, cur_stream(h), slabs.data_ptr(), 1);
  else
    launch_norm_bwd(to_dtype(h.scalar_type()), slabs.data_ptr<float>(), 1, h.data_ptr(), inv.data_ptr<float>(),
                    go.data_ptr<float>(), dh.data_ptr(), P.g, cur_stream(h));
  return dh;
}

// ---- ring-negatives stage ops (O(local) memory; parallel/ring.py) --------------------------
// `zq_chunk` holds the normalised rows of ONE rank (rows_pad x op_ld): the rank whose global
// column tiles start at `b_tile0`. `tiles` is an explicit int32 [n, 4] tile list (a subset of
// the plan's forward tiles).
static const int4* tile_ptr(const at::Tensor& tiles, int& n) {
  check_input(tiles, "tiles");
  NTXENT_CHECK(tiles.dim() == 2 && tiles.size(1) == 4 && tiles.scalar_type() == at::kInt, "tiles must be int32 [n, 4]");
  n = (int)tiles.size(0);
  return reinterpret_cast<const int4*>(tiles.data_ptr<int>());
}

void fwd_stats_tiles(const at::Tensor& zq_local, const at::Tensor& zq_chunk, int b_tile0, const at::Tensor& tiles,
                     const Plan& P, at::Tensor& part, int reserve_cus) {
  check_input(zq_local, "zq_local");
  check_input(zq_chunk, "zq_chunk");
  check_input(part, "part");
  NTXENT_CHECK(zq_chunk.numel() == (long)P.g.rows_pad * P.op_ld(), "zq_chunk must be one rank's [rows_pad, ld] rows");
  NTXENT_CHECK(part.numel() == (long)P.g.col_tiles * P.g.rows_pad * 2 && part.scalar_type() == at::kFloat,
               "part must be float32 [col_tiles, rows_pad, 2]");
  int n = 0;
  const int4* tp = tile_ptr(tiles, n);
  if (n == 0) return;
  const at::DeviceGuard guard(zq_local.device());
  auto ws = gemm_ws(zq_local, n, P, reserve_cus);
  BlockView bv;
  bv.b_tile0 = b_tile0;
  launch_fwd_stats(P.comp, zq_local.data_ptr(), zq_chunk.data_ptr(), tp, n,
                   reinterpret_cast<float2*>(part.data_ptr<float>()), nullptr, ws, P.g, cur_stream(zq_local), bv);
}

// Coefficient tiles of one column block (recomputed S) into a compact [row_tiles][c_ld] tile
// buffer whose first column tile is global tile c_tile0.
at::Tensor coef_gemm_tiles(const at::Tensor& zq_local, const at::Tensor& zq_chunk, int b_tile0, const at::Tensor& tiles,
                           const at::Tensor& lse2_all, const at::Tensor& cpos, const Plan& P, int c_ld, int c_tile0,
                           int reserve_cus) {
  check_input(zq_local, "zq_local");
  check_input(zq_chunk, "zq_chunk");
  NTXENT_CHECK(c_ld > 0, "c_ld must be positive");
  int n = 0;
  const int4* tp = tile_ptr(tiles, n);
  const at::DeviceGuard guard(zq_local.device());
  auto cbuf = at::empty({(long)P.g.row_tiles * c_ld * kTileElems}, opts(zq_local, to_scalar(P.bwd())));
  if (n == 0) return cbuf;
  auto ws = gemm_ws(zq_local, n, P, reserve_cus);
  BlockView bv;
  bv.b_tile0 = b_tile0;
  bv.c_ld = c_ld;
  bv.c_tile0 = c_tile0;
  launch_coef_gemm(P.comp, zq_local.data_ptr(), zq_chunk.data_ptr(), cbuf.data_ptr(), lse2_all.data_ptr<float>(),
                   cpos.data_ptr<float>(), tp, n, ws, P.g, cur_stream(zq_local), bv);
  return cbuf;
}

// dZ contribution of one column block: slabs = C_block [rows_pad x rows_pad] * Z_chunk, with
// zqt_chunk = that rank's [dim_n, ld_t] transposed rows (a one-block, world-1 geometry).
at::Tensor dz_block(const at::Tensor& cbuf_block, const at::Tensor& zqt_chunk, const Plan& P, int reserve_cus) {
  check_input(cbuf_block, "cbuf_block");
  check_input(zqt_chunk, "zqt_chunk");
  NTXENT_CHECK(zqt_chunk.numel() == (long)P.g.dim_n * P.g.ld_t, "zqt_chunk must be [dim_n, ld_t]");
  NTXENT_CHECK(cbuf_block.numel() == (long)P.g.row_tiles * P.g.row_tiles * kTileElems, "cbuf_block must be row_tiles^2 tiles");
  const at::DeviceGuard guard(cbuf_block.device());
  Geometry g1 = P.g;
  g1.world = 1;
  g1.rank = 0;
  g1.col_tiles = g1.row_tiles;
  auto slabs = at::empty({1, P.g.rows_pad, P.g.dim_n}, opts(cbuf_block, at::kFloat));
  auto ws = gemm_ws(cbuf_block, P.n_dz, P, reserve_cus);
  launch_dz(P.bwd(), cbuf_block.data_ptr(), zqt_chunk.data_ptr(), reinterpret_cast<const int4*>(P.dz_tiles.data_ptr<int>()),
            P.n_dz, slabs.data_ptr<float>(), ws, g1, cur_stream(cbuf_block));
  return slabs;
}

// ---- symmetric data-parallel step (sym_step.h; parallel/symmetric.py, parallel/emulate.py) ----
// The schedule and the launches are sym_step.cpp's. SymStep is what Python caches per shape: the
// SymPlan and its two device tile lists, uploaded once. Every phase takes the plan (for the
// temperature) and a bundle {name: tensor} of the SymBuffers it needs; sym_bufs checks each
// tensor's dtype and byte size against the plan before its pointer goes anywhere.
struct SymStep {
  SymPlan sp;
  Geometry g;
  int device = 0;
  at::Tensor fwd_tiles, dz_rows;
};

static std::shared_ptr<SymStep> sym_step(const Plan& P) {
  auto S = std::make_shared<SymStep>();
  S->sp = make_sym_plan(P.g, P.bwd(), P.comp == DType::FP8);
  S->g = P.g;
  S->device = P.device;
  S->fwd_tiles = upload_tiles(build_sym_fwd_tiles(P.g, S->sp.jobs, S->sp.nchunks), P.device);
  S->dz_rows = upload_tiles(S->sp.dz_rows, P.device);
  return S;
}

struct SymBundle {
  SymBuffers b;
  at::Tensor like;       // any tensor of the bundle (device, stream)
  size_t own_bytes = 0;
  DType in = DType::BF16;
};

static SymBundle sym_bufs(const SymStep& S, const Plan& P, const pybind11::dict& d) {
  const Geometry& g = P.g;
  const SymPlan& sp = S.sp;
  NTXENT_CHECK(g.rows == S.g.rows && g.dim == S.g.dim && g.world == S.g.world && g.rank == S.g.rank && P.device == S.device &&
                   P.bwd() == sp.bwd && (P.comp == DType::FP8) == sp.f8, "symmetric step: plan does not match");
  SymBundle r;
  size_t seen = 0;
  auto take = [&](const char* key, at::ScalarType t, size_t bytes, size_t* at_least = nullptr) -> void* {
    if (!d.contains(key)) return nullptr;
    at::Tensor x = d[key].cast<at::Tensor>();
    check_input(x, key);
    NTXENT_CHECK(x.scalar_type() == t && (at_least ? x.nbytes() >= bytes : x.nbytes() == bytes),
                 std::string(key) + ": wrong dtype or size for this symmetric plan");
    if (at_least) *at_least = x.nbytes();
    ++seen;
    r.like = x;
    return x.data_ptr();
  };
  const auto st = to_scalar(sp.bwd), ct = sp.contrib_f16 ? at::kHalf : at::kFloat;
  const size_t W = g.world, Rp = g.rows_pad, cs = dtype_size(sp.bwd), f2 = sizeof(float2);
  SymBuffers& b = r.b;
  if (d.contains("h")) {
    r.in = to_dtype(d["h"].cast<at::Tensor>().scalar_type());
    b.h = take("h", to_scalar(r.in), (size_t)g.rows * g.dim * dtype_size(r.in));
    b.dh = take("dh", to_scalar(r.in), (size_t)g.rows * g.dim * dtype_size(r.in));
  }
  b.zq_all = take("zq_all", st, W * Rp * g.ld_k * cs);
  b.zq8_all = take("zq8_all", at::kByte, W * Rp * g.ld_k8);
  b.zqt_all = take("zqt_all", st, W * g.dim_n * g.ld_t * cs);
  b.inv = static_cast<float*>(take("inv", at::kFloat, (size_t)g.rows * 4));
  b.ypos = static_cast<float*>(take("ypos", at::kFloat, (size_t)g.rows * 4));
  b.part = static_cast<float2*>(take("part", at::kFloat, g.col_tiles * Rp * f2));
  b.part_x = static_cast<float2*>(take("part_x", at::kFloat, sp.bytes.part_x));
  b.sbuf = take("sbuf", st, sp.bytes.sbuf);
  b.cbuf = take("cbuf", st, sp.bytes.cbuf);
  b.mbuf = take("mbuf", st, sp.bytes.mbuf);
  b.lse2_all = static_cast<float*>(take("lse2_all", at::kFloat, W * Rp * 4));
  b.cpos = static_cast<float*>(take("cpos", at::kFloat, Rp * 4));
  b.loss = static_cast<float*>(take("loss", at::kFloat, 4));
  b.contrib = take("contrib", ct, sp.bytes.contrib);
  // the own dZ needs the own slab; the normalisation backward checks the whole stack (sym_norm_bwd)
  b.own = static_cast<float*>(take("own", at::kFloat, Rp * g.dim_n * 4, &r.own_bytes));
  b.recv = take("recv", at::kHalf, sp.bytes.recv);
  b.grad_out = static_cast<const float*>(take("grad_out", at::kFloat, 4));
  NTXENT_CHECK(seen == d.size() && seen > 0, "symmetric step: unknown or no buffer in the bundle");
  b.fwd_tiles = reinterpret_cast<const int4*>(S.fwd_tiles.data_ptr<int>());
  b.dz_rows = reinterpret_cast<const int4*>(S.dz_rows.data_ptr<int>());
  return r;
}

// a phase as a method of SymStep: (plan, bundle, extra arguments...) on the bundle's device and stream
template <class... A, class F>
static auto sym_phase(F run) {
  return [run](const SymStep& S, const Plan& P, const pybind11::dict& d, A... a) {
    SymBundle x = sym_bufs(S, P, d);
    const at::DeviceGuard guard(x.like.device());
    run(S, P, x, cur_stream(x.like), a...);
  };
}

// the schedule as Python reads it: lists of tuples in the field order of sym_step.h
static pybind11::dict sym_plan_dict(const SymPlan& p) {
  namespace py = pybind11;
  auto jobs = [](const std::vector<SymJob>& v) {
    py::list l;
    for (const SymJob& j : v) l.append(py::make_tuple(j.q, j.m0, j.m1, j.k0, j.k1));
    return l;
  };
  auto xfers = [](const std::vector<SymXfer>& v) {
    py::list l;
    for (const SymXfer& x : v) l.append(py::make_tuple(x.send, x.peer, x.slot0, x.slot1, x.t0, x.t1, x.pack_off));
    return l;
  };
  auto calls = [](const std::vector<SymDzCall>& v) {
    py::list l;
    for (const SymDzCall& c : v)
      l.append(py::make_tuple(c.mirror, c.a_tile0, c.a_panel_tiles, c.b_block0, c.b_col0, c.b_kblk_cols, c.k_tiles, c.m0, c.m1,
                              c.out, c.accum, c.rows_off));
    return l;
  };
  py::dict r, nb;
  r["world"] = p.world; r["rank"] = p.rank; r["row_tiles"] = p.row_tiles; r["contrib_f16"] = p.contrib_f16;
  r["jobs"] = jobs(p.jobs); r["incoming"] = jobs(p.incoming);
  r["nchunks"] = p.nchunks; r["nfull"] = p.nfull; r["split"] = p.split;
  r["n_own"] = p.n_own; r["n_fwd"] = p.n_fwd; r["c_ld"] = p.c_ld;
  py::list segs, rows, dzr;
  for (const auto& sg : p.segs) segs.append(py::make_tuple(sg.first, sg.second));
  for (const auto& c : p.rows) rows.append(xfers(c));
  for (const int4& t : p.dz_rows) dzr.append(py::make_tuple(t.x, t.y));
  r["segs"] = segs; r["rows"] = rows; r["rows_f16"] = xfers(p.rows_f16);
  r["col_partials"] = xfers(p.col_partials); r["contribs"] = xfers(p.contribs);
  r["partner_dz"] = calls(p.partner_dz); r["own_dz"] = calls(p.own_dz); r["dz_rows"] = dzr;
  nb["sbuf"] = p.bytes.sbuf; nb["cbuf"] = p.bytes.cbuf; nb["mbuf"] = p.bytes.mbuf; nb["part_x"] = p.bytes.part_x;
  nb["slab"] = p.bytes.slab; nb["contrib"] = p.bytes.contrib; nb["recv"] = p.bytes.recv; nb["own"] = p.bytes.own;
  nb["xsend"] = p.bytes.xsend; nb["xrecv"] = p.bytes.xrecv; nb["dz_rows"] = p.bytes.dz_rows;
  r["bytes"] = nb;
  return r;
}

// A general dZ view as a stage op (the symmetric step resolves its own calls in sym_step.cpp; this
// one serves a plain GEMM with reserved CUs, tests/test_gpu_production.py):
// out[row tiles m0..m1) (+)= A * B with A = tiles of `abuf` starting at tile index a_tile0 (row
// panels a_panel_tiles tiles apart; row tile mt at a_tile0 + mt * a_panel_tiles), K = k_tiles * 256
// columns of B = `bbuf` (ZqT blocks [nblk, dim_n, ld_t], or one [dim_n, ld_t]) starting at block
// b_block0, column b_col0; a K range longer than one block runs over consecutive whole blocks.
// `out` is float32 [>= m1 * 256, dim_n] (row tiles may exceed row_tiles: stacked outputs).
void dz_view(const at::Tensor& abuf, long a_tile0, long a_panel_tiles, const at::Tensor& bbuf, int b_block0, long b_col0,
             int k_tiles, int m0, int m1, at::Tensor& out, bool accum, const Plan& P, int reserve_cus) {
  check_input(abuf, "abuf");
  check_input(bbuf, "bbuf");
  check_input(out, "out");
  const auto st = to_scalar(P.bwd());
  NTXENT_CHECK(abuf.scalar_type() == st && bbuf.scalar_type() == st, "operands must be in the backward dtype");
  NTXENT_CHECK(0 <= m0 && m0 <= m1, "bad row tile range");
  NTXENT_CHECK(k_tiles >= 0 && a_panel_tiles >= k_tiles && a_tile0 >= 0, "bad A view");
  if (m1 > m0)
    NTXENT_CHECK(a_tile0 + (long)(m1 - 1) * a_panel_tiles + k_tiles <= abuf.numel() / kTileElems, "A view out of bounds");
  const long blk = (long)P.g.dim_n * P.g.ld_t;
  NTXENT_CHECK(bbuf.numel() % blk == 0, "bbuf must be [nblk, dim_n, ld_t]");
  const long nblk = bbuf.numel() / blk;
  const long kcols = (long)k_tiles * kTile;
  long kblk_cols = kcols;
  if (b_col0 + kcols > P.g.rows_pad) {  // spans whole rank blocks
    NTXENT_CHECK(b_col0 == 0 && kcols % P.g.rows_pad == 0, "multi-block K ranges must cover whole blocks");
    kblk_cols = P.g.rows_pad;
  }
  const long nspan = (kcols + kblk_cols - 1) / kblk_cols;
  NTXENT_CHECK(b_block0 >= 0 && b_block0 + nspan <= nblk && b_col0 >= 0, "B view out of bounds");
  const bool out_f16 = out.scalar_type() == at::kHalf;
  NTXENT_CHECK((out.scalar_type() == at::kFloat || out_f16) && out.dim() == 2 && out.size(1) == P.g.dim_n &&
                   out.size(0) >= (long)m1 * kTile, "out must be float32 or float16 [>= m1*256, dim_n]");
  NTXENT_CHECK(!(out_f16 && accum), "fp16 output cannot accumulate");
  if (m1 == m0 || k_tiles == 0) return;
  const at::DeviceGuard guard(abuf.device());
  at::Tensor sub;
  {
    static std::mutex mu;
    static std::map<std::tuple<int, int, int, int>, at::Tensor> cache;
    std::lock_guard<std::mutex> lock(mu);
    auto& c = cache[{P.device, P.g.dim_n, m0, m1}];
    if (!c.defined()) {
      std::vector<int4> v;
      for (int ti = m0; ti < m1; ++ti)
        for (int tn = 0; tn < P.g.dim_n / kTile; ++tn) v.push_back(make_int4(ti, tn, 0, 0));
      c = upload_tiles(v, P.device);
    }
    sub = c;
  }
  const long cs = (long)dtype_size(P.bwd());
  const char* a = static_cast<const char*>(abuf.data_ptr()) + a_tile0 * kTileElems * cs;
  const char* b = static_cast<const char*>(bbuf.data_ptr()) + ((long)b_block0 * blk + b_col0) * cs;
  auto ws = gemm_ws(abuf, (int)sub.size(0), P, reserve_cus);
  launch_dz_view(P.bwd(), a, a_panel_tiles, b, kblk_cols, blk, k_tiles, reinterpret_cast<const int4*>(sub.data_ptr<int>()),
                 (int)sub.size(0), out.data_ptr(), accum, ws, P.g, cur_stream(abuf), out_f16);
}

// ---- single-process fused flows ------------------------------------------------------
// The step itself is step.cpp's (shared with the native Engine): these two resolve its plan,
// allocate its buffers from torch's allocator (self-cleaning counters: the per-stream
// device_scratch slots) and keep the tuple the autograd Function saves.

// at::empty of `bytes` in dtype t (ld > 0: rows of ld elements), its pointer stored in dst
template <class T>
static at::Tensor mk(T*& dst, const at::Tensor& like, size_t bytes, at::ScalarType t, long ld = 0) {
  const long n = (long)(bytes / c10::elementSize(t));
  at::Tensor x = ld > 0 ? at::empty({n / ld, ld}, opts(like, t)) : at::empty({n}, opts(like, t));
  dst = static_cast<T*>(x.data_ptr());
  return x;
}
static void* scratch(const at::Tensor& like, size_t bytes, int slot) { return device_scratch(like, bytes, slot).data_ptr(); }

static StepBuffers step_buffers(const at::Tensor& h, const Plan& P, const StepPlan& sp, const StepBufferBytes& nb) {
  StepBuffers b;
  b.h = h.data_ptr();
  b.fwd_tiles = reinterpret_cast<const int4*>(P.fwd_tiles.data_ptr<int>());
  b.dz_tiles = reinterpret_cast<const int4*>(P.dz_tiles.data_ptr<int>());
  if (sp.small) {
    b.small_scratch = scratch(h, nb.small_scratch, 2);
  } else {
    b.ws.num_cus = sp.num_cus;
    b.ws.bytes = nb.ws;
    b.ws.ptr = scratch(h, nb.ws, 0);
  }
  return b;
}

// Returns {loss, zq, zqt, inv, lse2, sc, cpos}, whose layout tells the backward what ran:
//   small path: zqt undefined, cpos = a_i (the backward recomputes S from zq);
//   raw-operand forward: zq empty (0 elements, the backward dtype: nothing reads unit rows);
//   fp8 backward: zqt = e4m3(256 Zq^T) as uint8, cpos = [cpos | mneg2 (Rpad) | lmin] (Q8Stats);
//   fp8 forward with the fp16 backward: 64 spare cpos entries (the backward sees fp16 rows);
//   sc: the kept cosines (keep_cos; always on fp8 plans), else undefined.
std::vector<at::Tensor> fused_forward(const at::Tensor& h, double T, const std::string& compute, bool keep_cos) {
  check_input(h, "h");
  check_stacked(h, "z");
  const at::DeviceGuard guard(h.device());
  // "auto" = the input-dtype policy (fp32 stays exact); mixed precision is requested by the
  // callers as an explicit "fp16".
  const DType comp = choose_compute(h.scalar_type(), false, compute);
  auto P = get_plan((int)h.size(0), (int)h.size(1), 1, 0, T, dtype_name(comp), h.device().index());
  const Geometry& g = P->g;
  const StepPlan sp =
      resolve_step_plan(g, to_dtype(h.scalar_type()), comp, keep_cos || comp == DType::FP8, P->num_cus);
  const StepBufferBytes nb = step_buffer_bytes(sp);
  const auto bt = to_scalar(sp.bwd);
  StepBuffers b = step_buffers(h, *P, sp, nb);
  at::Tensor zq8, zqt, ypos, part, sc, fold_pre;
  auto inv = mk(b.inv, h, nb.inv, at::kFloat);
  auto lse2 = mk(b.lse2, h, nb.lse2, at::kFloat);
  auto loss = at::empty({}, opts(h, at::kFloat));
  b.loss = loss.data_ptr<float>();
  auto cpos = mk(b.cpos, h, nb.cpos + nb.q8_mneg + (sp.f8 ? 64 * 4 : 0), at::kFloat);
  auto zq = sp.raw ? at::empty({0}, opts(h, bt)) : mk(b.zq, h, nb.zq, bt, g.ld_k);
  if (!sp.small || !sp.small_fwd_fused) ypos = mk(b.ypos, h, nb.ypos, at::kFloat);
  if (!sp.small) {
    if (sp.raw) {
      fold_pre = mk(b.fold_pre, h, nb.fold_pre, at::kFloat);
      b.fold_cnt = static_cast<int*>(scratch(h, nb.fold_cnt, 3));
    }
    if (sp.f8) zq8 = mk(b.zq8, h, nb.zq8, at::kByte, g.ld_k8);
    // ZqT (the dZ GEMM's B operand) is first read in the backward: the forward or the LSE launch
    // writes it beside its own work (one stream: a side-stream transpose cost an event record and
    // a join of ~5-7 us each, or stretched the forward GEMM when launched beside it).
    zqt = sp.q8 ? mk(b.zq8t, h, nb.zq8t, at::kByte, q8_ldt(g)) : mk(b.zqt, h, nb.zqt, bt, g.ld_t);
    part = mk(b.part, h, nb.part, at::kFloat);
    if (sp.keep_cos) sc = mk(b.sbuf, h, nb.sbuf, bt);
    if (sp.q8) {
      b.q8_mneg = b.cpos + g.rows_pad;
      b.q8_lmin = b.cpos + 2 * (size_t)g.rows_pad;
    }
    b.block_loss = static_cast<float*>(scratch(h, nb.block_loss, 1));
  }
  step_forward(sp, b, cur_stream(h));
  return {loss, zq, zqt, inv, lse2, sc, cpos};
}

// want_tau: also dL/dtau (StepPlan::tau_grad), a 0-d fp32 tensor; undefined otherwise.
static std::pair<at::Tensor, at::Tensor> fused_backward_impl(
    const at::Tensor& h, const at::Tensor& zq, const c10::optional<at::Tensor>& zqt_in, const at::Tensor& inv,
    const at::Tensor& lse2, const c10::optional<at::Tensor>& sc_in, const at::Tensor& cpos, const at::Tensor& grad_out,
    double T, bool want_tau) {
  const at::DeviceGuard guard(h.device());
  const DType rows_dt = to_dtype(zq.scalar_type());
  auto P = get_plan((int)h.size(0), (int)h.size(1), 1, 0, T, dtype_name(rows_dt), h.device().index());
  const Geometry& g = P->g;
  const at::Tensor zqt = zqt_in.has_value() ? *zqt_in : at::Tensor();
  const at::Tensor sc = sc_in.has_value() ? *sc_in : at::Tensor();
  // what the forward ran, read off the tuple's layout (see fused_forward)
  const bool q8 = zqt.defined() && zqt.scalar_type() == at::kByte;
  const bool f8 = zqt.defined() && cpos.numel() != g.rows_pad;
  StepOverrides ov;
  ov.small_path = !zqt.defined();
  ov.fp8_backward = q8;
  // (sc undefined: a second backward (retain_graph), which recomputes the cosines)
  StepPlan sp = resolve_step_plan(g, to_dtype(h.scalar_type()), f8 ? DType::FP8 : rows_dt, sc.defined(),
                                  P->num_cus, ov);
  sp.tau_grad = want_tau;
  NTXENT_CHECK(sp.small == !zqt.defined(), "fused_backward: missing ZqT for a large-problem plan");
  NTXENT_CHECK(sp.q8 == q8 && (!q8 || cpos.numel() == 2 * (long)g.rows_pad + 64),
               "fused_backward (fp8): kept cosines and the forward's Q8Stats required");
  const StepBufferBytes nb = step_buffer_bytes(sp);
  StepBuffers b = step_buffers(h, *P, sp, nb);
  auto go = grad_scalar(grad_out);
  auto dh = at::empty_like(h);
  b.inv = static_cast<float*>(inv.data_ptr());
  b.lse2 = static_cast<float*>(lse2.data_ptr());
  b.cpos = static_cast<float*>(cpos.data_ptr());
  at::Tensor zr = zq, cb, dotp, dot, slabs, dtau;
  if (!sp.small) {
    // (a raw-operand forward returns no unit rows: a second backward rebuilds them to recompute S)
    if (!sp.keep_cos && zq.numel() == 0) zr = prep(h, *P, c10::nullopt, c10::nullopt)[0];
    cb = mk(b.cbuf, h, nb.cbuf, sp.q8 ? at::kByte : to_scalar(sp.bwd));
    slabs = mk(b.slabs, h, nb.slabs, sp.bwd != DType::F32 ? at::kHalf : at::kFloat);
    if (sp.fuse) {
      dotp = mk(b.dotp, h, nb.dotp, at::kFloat);
      dot = mk(b.dot, h, nb.dot, at::kFloat);
    }
    if (sp.dfold) b.dot_cnt = static_cast<int*>(scratch(h, nb.dot_cnt, 4));
    (q8 ? b.zq8t : b.zqt) = zqt.data_ptr();
    if (q8) {
      b.q8_mneg = b.cpos + g.rows_pad;
      b.q8_lmin = b.cpos + 2 * (size_t)g.rows_pad;
    }
    b.sbuf = sc.defined() ? sc.data_ptr() : nullptr;
  }
  if (sp.tau_grad) {  // the unfused and the small paths store their per-row dot as well
    if (!dot.defined()) dot = mk(b.dot, h, nb.dot, at::kFloat);
    dtau = at::empty({}, opts(h, at::kFloat));
    b.dtau = dtau.data_ptr<float>();
  }
  b.zq = zr.data_ptr();
  b.grad_out = go.data_ptr<float>();
  b.dh = dh.data_ptr();
  step_backward(sp, b, cur_stream(h));
  return {dh, dtau};
}

at::Tensor fused_backward(const at::Tensor& h, const at::Tensor& zq, const c10::optional<at::Tensor>& zqt_in,
                          const at::Tensor& inv,
                          const at::Tensor& lse2, const c10::optional<at::Tensor>& sc_in, const at::Tensor& cpos,
                          const at::Tensor& grad_out, double T) {
  return fused_backward_impl(h, zq, zqt_in, inv, lse2, sc_in, cpos, grad_out, T, false).first;
}

// fused_backward plus the temperature gradient: (dh, dtau), dtau = dL/dtau times grad_out, a 0-d
// fp32 tensor. dh is bitwise fused_backward's.
std::tuple<at::Tensor, at::Tensor> fused_backward_tau(const at::Tensor& h, const at::Tensor& zq,
                                                      const c10::optional<at::Tensor>& zqt_in, const at::Tensor& inv,
                                                      const at::Tensor& lse2, const c10::optional<at::Tensor>& sc_in,
                                                      const at::Tensor& cpos, const at::Tensor& grad_out, double T) {
  auto r = fused_backward_impl(h, zq, zqt_in, inv, lse2, sc_in, cpos, grad_out, T, true);
  return {r.first, r.second};
}

// ---- reference-compatible API (src/binding_new.cpp:5-20) -------------------------------
at::Tensor forward_op(const at::Tensor& z, double T, bool use_mixed_precision) {
  auto out = fused_forward(z.contiguous(), T, use_mixed_precision ? "fp16" : "auto", /*keep_cos=*/false);
  return out[0];
}

// Row statistics handed from forward_with_stats to backward. The backward trusts a caller's LSE
// only when it is exactly a tensor forward_with_stats returned, unmodified since, for the SAME z
// tensor (same TensorImpl, same version counter: no in-place update in between), the same T and
// the same precision; anything else (the reference's softmax, an empty tensor, a stale LSE from
// an earlier step or another temperature) makes the backward recompute the statistics, so a
// result never silently depends on stale caller-provided stats.
namespace {
struct StatsTag {
  c10::weak_intrusive_ptr<c10::TensorImpl> stats, z;
  int64_t stats_ver = 0, z_ver = 0;
  double T = 0.0;
  bool mp = false;
};
std::mutex g_tag_mu;
std::vector<StatsTag> g_tags;  // most recent last; bounded
constexpr size_t kMaxTags = 32;

void tag_stats(const at::Tensor& stats, const at::Tensor& z, double T, bool mp) {
  std::lock_guard<std::mutex> lock(g_tag_mu);
  g_tags.erase(std::remove_if(g_tags.begin(), g_tags.end(), [](const StatsTag& t) { return t.stats.expired(); }),
               g_tags.end());
  if (g_tags.size() >= kMaxTags) g_tags.erase(g_tags.begin());
  g_tags.push_back(StatsTag{c10::weak_intrusive_ptr<c10::TensorImpl>(stats.getIntrusivePtr()),
                            c10::weak_intrusive_ptr<c10::TensorImpl>(z.getIntrusivePtr()), stats._version(),
                            z._version(), T, mp});
}

bool stats_match(const at::Tensor& stats, const at::Tensor& z, double T, bool mp) {
  if (!stats.defined() || !z.defined()) return false;
  std::lock_guard<std::mutex> lock(g_tag_mu);
  for (auto it = g_tags.rbegin(); it != g_tags.rend(); ++it) {
    auto sp = it->stats.lock();
    if (!sp || sp.get() != stats.unsafeGetTensorImpl()) continue;
    auto zp = it->z.lock();
    return zp && zp.get() == z.unsafeGetTensorImpl() && it->z_ver == z._version() &&
           it->stats_ver == stats._version() && it->T == T && it->mp == mp;
  }
  return false;
}
}  // namespace

std::vector<at::Tensor> forward_with_stats(const at::Tensor& z, double T, bool use_mixed_precision) {
  auto out = fused_forward(z.contiguous(), T, use_mixed_precision ? "fp16" : "auto", false);
  const int R = (int)z.size(0);
  auto lse_nat = out[4].narrow(0, 0, R) * (float)0.6931471805599453;
  tag_stats(lse_nat, z, T, use_mixed_precision);
  return {out[0], lse_nat};
}

// backward(z, stats, grad_out, T): the reference passes a softmax matrix here that its own
// forward never returns (src/ntxent_kernel.cu:202). Here `stats` may be the per-row LSE that
// forward_with_stats returned for this z (see StatsTag): the backward then costs ONE similarity
// GEMM (the cosines are recomputed inside the coefficient GEMM; a stateless op keeps none).
// Anything else in that slot is ignored and the row statistics are recomputed (one more
// similarity GEMM).
// Returns (grad_z, grad_logits). grad_logits = dL/dS [2N, 2N] (fp32) is a debug/parity output
// built only when want_grad_logits is set; otherwise it is an empty tensor, so the default call
// runs no extra GEMM and allocates nothing quadratic.
std::tuple<at::Tensor, at::Tensor> backward_op(const at::Tensor& z_in, const at::Tensor& stats,
                                               const at::Tensor& grad_out, double T, bool use_mixed_precision,
                                               bool want_grad_logits) {
  auto z = z_in.contiguous();
  const at::DeviceGuard guard(z.device());
  const DType comp = choose_compute(z.scalar_type(), use_mixed_precision, "");
  auto P = get_plan((int)z.size(0), (int)z.size(1), 1, 0, T, dtype_name(comp), z.device().index());
  auto pr = prep(z, *P, c10::nullopt, c10::nullopt);
  auto zqt = transpose(pr[0], *P, c10::nullopt);
  const long R = z.size(0), n = R / 2, Rp = P->g.rows_pad;
  at::Tensor lse2, cpos;
  const bool have_lse = stats.defined() && stats.dim() == 1 && stats.size(0) == R && stats.is_floating_point() &&
                        stats.device() == z.device() && stats_match(stats, z_in, T, use_mixed_precision);
  if (have_lse) {
    // lse2 in log2 units; C_i,p(i) = -(a_i + a_p(i)), a_i = 1 - P_ip = -expm1(y_ip - lse_i)
    // (expm1 keeps a_i accurate when P_ip -> 1)
    auto lse_nat = stats.to(at::kFloat);
    lse2 = at::zeros({Rp}, opts(z, at::kFloat));
    lse2.narrow(0, 0, R).copy_(lse_nat * (float)1.4426950408889634);
    auto y_nat = pr[2].narrow(0, 0, R) * (float)0.6931471805599453;
    auto a = -at::expm1(y_nat - lse_nat);
    cpos = at::zeros({Rp}, opts(z, at::kFloat));
    cpos.narrow(0, 0, R).copy_(-(a + at::roll(a, {n})));
  } else {
    lse2 = at::empty({Rp}, opts(z, at::kFloat));
    cpos = at::empty({Rp}, opts(z, at::kFloat));
    auto fs = fwd_stats(pr[0], pr[0], *P, false);
    lse(fs[0], pr[2], lse2, cpos, *P);
  }
  auto sc = coef_gemm(pr[0], pr[0], lse2, cpos, *P);
  auto slabs = dz(sc, zqt, *P);
  auto go = grad_scalar(grad_out);
  auto dh = norm_bwd(slabs, z, pr[1], go, *P);
  at::Tensor grad_logits;
  if (want_grad_logits) {
    // dL/dS_ij = grad_out * (P_ij - [j == p(i)]) / 2N  (debug/parity output)
    auto zf = z.to(at::kFloat);
    auto zn = zf / zf.norm(2, {1}, true).clamp_min(1e-12);
    auto S = at::matmul(zn, zn.t()) / T;
    S.fill_diagonal_(-std::numeric_limits<float>::infinity());
    auto lse_nat = lse2.narrow(0, 0, R) * (float)0.6931471805599453;
    auto G = at::exp(S - lse_nat.unsqueeze(1));
    auto idx = at::arange(R, opts(z, at::kLong));
    auto pos = (idx + n) % R;
    G.index_put_({idx, pos}, G.index({idx, pos}) - 1.0);
    grad_logits = G * (go / (double)R);
  } else {
    grad_logits = at::empty({0}, opts(z, at::kFloat));
  }
  return {dh, grad_logits};
}

bool check_tensor_core_support() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  return check_matrix_core_support(dev);
}


// ---- the native Engine from Python (ntxent_amd.native) ------------------------------------
// The libtorch-free runtime (engine.h: one arena, fixed launch sequence, hipGraph capture,
// RcclComm data parallelism) driven from torch tensors on the current stream. The RCCL unique
// id is produced by rccl_unique_id() on one rank and handed to the others by the caller
// (ntxent_amd.native bootstraps it through the torch.distributed store).
namespace {
DType parse_dtype_name(const std::string& s) {
  if (s == "float32" || s == "fp32") return DType::F32;
  if (s == "float16" || s == "fp16") return DType::F16;
  if (s == "bfloat16" || s == "bf16") return DType::BF16;
  if (s == "fp8" || s == "e4m3") return DType::FP8;
  throw std::invalid_argument("unknown dtype '" + s + "' (fp32|fp16|bf16|fp8)");
}

class NativeEngine {
 public:
  NativeEngine(int rows, int dim, double T, const std::string& input, const std::string& compute,
               const std::string& negatives, int rank, int world, const std::string& uid, int device, bool keep_cos,
               int comm_reserve_cus, std::shared_ptr<RcclComm> comm = nullptr, bool temperature_grad = false)
      : device_(device) {
    NTXENT_CHECK(world >= 1 && rank >= 0 && rank < world, "NativeEngine: bad rank/world");
    NTXENT_CHECK(negatives == "symmetric" || negatives == "allgather", "negatives must be symmetric|allgather");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(device);
    if (comm) {  // a communicator shared by every engine of this process group (one RCCL init)
      NTXENT_CHECK(comm->rank() == rank && comm->world() == world, "NativeEngine: communicator rank/world mismatch");
      comm_ = std::move(comm);
    } else if (world > 1) {
      comm_ = std::make_shared<RcclComm>(rank, world, uid, device);
    }
    EngineConfig cfg;
    cfg.rows = rows;
    cfg.dim = dim;
    cfg.temperature = (float)T;
    cfg.input = parse_dtype_name(input);
    NTXENT_CHECK(cfg.input != DType::FP8, "NativeEngine: input must be fp32|fp16|bf16");
    cfg.compute = compute == "auto" ? (cfg.input == DType::F32 ? DType::F32 : DType::F16) : parse_dtype_name(compute);
    cfg.keep_cos = keep_cos;
    cfg.comm_reserve_cus = comm_reserve_cus;
    cfg.negatives = negatives == "symmetric" ? Negatives::kSymmetric : Negatives::kAllGather;
    cfg.device = device;
    cfg.temperature_grad = temperature_grad;
    in_ = to_scalar(cfg.input);
    eng_ = std::make_unique<Engine>(cfg, comm_.get());
  }

  void forward(const at::Tensor& h) {
    check_h(h);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(device_);
    h_ = h;  // the backward reads the forward's h
    eng_->forward(h.data_ptr(), cur_stream(h));
  }
  at::Tensor backward(const c10::optional<at::Tensor>& grad_out) {
    NTXENT_CHECK(h_.defined(), "NativeEngine.backward needs a preceding forward");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(device_);
    at::Tensor go;
    if (grad_out && grad_out->defined()) {
      go = grad_out->to(h_.device(), at::kFloat).reshape({1}).contiguous();
    }
    at::Tensor dh = at::empty_like(h_);
    eng_->backward(go.defined() ? go.data_ptr<float>() : nullptr, dh.data_ptr(), cur_stream(h_));
    return dh;
  }
  // the global mean loss as a 0-d fp32 tensor (stream-ordered copy of the engine's slot)
  at::Tensor loss_tensor() const {
    NTXENT_CHECK(h_.defined(), "no forward yet");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(device_);
    at::Tensor out = at::empty({}, h_.options().dtype(at::kFloat));
    NTXENT_HIP_CHECK(hipMemcpyAsync(out.data_ptr(), eng_->loss_device(), sizeof(float), hipMemcpyDeviceToDevice,
                                    cur_stream(h_)));
    return out;
  }
  std::tuple<at::Tensor, at::Tensor> step(const at::Tensor& h) {
    forward(h);
    at::Tensor dh = backward(c10::nullopt);
    return {loss_tensor(), dh};
  }
  // hipGraph of one step for fixed h (dh is returned and reused by every replay). The graph
  // holds h's and dh's device pointers, so both are kept alive in their own members (gh_, gdh_)
  // for as long as the graph exists, whatever forward()/step() do with h_ in between.
  // Single process only: a captured step of a multi-rank engine would bake RCCL calls into the
  // graph.
  at::Tensor capture(const at::Tensor& h) {
    check_h(h);
    NTXENT_CHECK(world() == 1, "NativeEngine.capture: single-process engines only (world == 1)");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(device_);
    at::Tensor dh = at::empty_like(h);
    eng_->capture(h.data_ptr(), dh.data_ptr(), cur_stream(h));
    gh_ = h;
    gdh_ = dh;
    h_ = h;  // loss_tensor() after a replay reads the graph's forward
    return gdh_;
  }
  void replay() {
    NTXENT_CHECK(eng_->captured() && gh_.defined(), "NativeEngine.replay needs capture()");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(device_);
    // the engine's backward reads the forward input: point it back at the captured one
    h_ = gh_;
    eng_->replay(cur_stream(gh_));
  }
  // world 1: the next forward / backward run at `t` (same arena); a captured graph is dropped
  void set_temperature(double t) {
    c10::hip::HIPGuardMasqueradingAsCUDA guard(device_);
    eng_->set_temperature((float)t);
    gh_ = at::Tensor();
    gdh_ = at::Tensor();
  }
  double temperature() const { return eng_->geometry().temperature; }
  bool captured() const { return eng_->captured(); }
  // dL/dtau of the last backward as a 0-d fp32 tensor (stream-ordered copy of the engine's slot)
  at::Tensor temperature_grad() const {
    NTXENT_CHECK(h_.defined(), "no backward yet");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(device_);
    const float* src = eng_->temperature_grad_device();
    NTXENT_CHECK(src != nullptr, "NativeEngine.temperature_grad: built without temperature_grad=True");
    at::Tensor out = at::empty({}, h_.options().dtype(at::kFloat));
    NTXENT_HIP_CHECK(hipMemcpyAsync(out.data_ptr(), src, sizeof(float), hipMemcpyDeviceToDevice, cur_stream(h_)));
    return out;
  }
  // Engine::positive_rank of this rank's rows h: {rank, pos_cos, hard_neg_cos}
  std::vector<at::Tensor> positive_rank(const at::Tensor& h) {
    check_h(h);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(device_);
    auto rank = at::empty({h.size(0)}, h.options().dtype(at::kInt));
    auto pos = at::empty({h.size(0)}, h.options().dtype(at::kFloat));
    auto hard = at::empty({h.size(0)}, h.options().dtype(at::kFloat));
    eng_->positive_rank(h.data_ptr(), rank.data_ptr<int>(), pos.data_ptr<float>(), hard.data_ptr<float>(),
                        cur_stream(h));
    return {rank, pos, hard};
  }
  size_t device_bytes() const { return eng_->device_bytes(); }
  bool symmetric() const { return eng_->symmetric(); }
  bool small() const { return eng_->small(); }
  int rank() const { return comm_ ? comm_->rank() : 0; }
  int world() const { return comm_ ? comm_->world() : 1; }

 private:
  void check_h(const at::Tensor& h) const {
    const auto& c = eng_->config();
    NTXENT_CHECK(h.is_cuda() && h.device().index() == device_, "h must be on the engine's device");
    NTXENT_CHECK(h.scalar_type() == in_, "h dtype does not match the engine's input dtype");
    NTXENT_CHECK(h.dim() == 2 && h.size(0) == c.rows && h.size(1) == c.dim && h.is_contiguous(),
                 "h must be a contiguous [rows, dim] tensor");
  }
  int device_ = 0;
  at::ScalarType in_ = at::kBFloat16;
  std::shared_ptr<RcclComm> comm_;  // declared before eng_: destroyed after it
  std::unique_ptr<Engine> eng_;
  at::Tensor h_;         // input of the last forward (read by backward)
  at::Tensor gh_, gdh_;  // the captured graph's input and output (alive while the graph exists)
};
}  // namespace

}  // namespace th
}  // namespace ntxent

// ---- torch.ops registration (python/test.py:137 resolves `torch.ops.ntxent_cuda`) -------
TORCH_LIBRARY(ntxent_cuda, m) {
  m.def("forward(Tensor z, float T, bool use_mixed_precision=False) -> Tensor");
  m.def("backward(Tensor z, Tensor softmax, Tensor grad_out, float T, bool use_mixed_precision=False, bool want_grad_logits=False) -> (Tensor, Tensor)");
  m.def("check_tensor_core_support() -> bool", &ntxent::th::check_tensor_core_support);
}
TORCH_LIBRARY_IMPL(ntxent_cuda, CUDA, m) {
  m.impl("forward", &ntxent::th::forward_op);
  m.impl("backward", &ntxent::th::backward_op);
}
TORCH_LIBRARY(ntxent, m) {
  m.def("forward(Tensor z, float T, bool use_mixed_precision=False) -> Tensor");
  m.def("forward_with_stats(Tensor z, float T, bool use_mixed_precision=False) -> Tensor[]");
  m.def("backward(Tensor z, Tensor softmax, Tensor grad_out, float T, bool use_mixed_precision=False, bool want_grad_logits=False) -> (Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(ntxent, CUDA, m) {
  m.impl("forward", &ntxent::th::forward_op);
  m.impl("forward_with_stats", &ntxent::th::forward_with_stats);
  m.impl("backward", &ntxent::th::backward_op);
}

// ---- pybind11 module ---------------------------------------------------------------------
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  namespace py = pybind11;
  using namespace ntxent::th;
  m.doc() = "MI355X (gfx950) NT-Xent loss: MFMA/LDS HIP kernels";
  py::class_<Plan, std::shared_ptr<Plan>>(m, "Plan")
      .def_property_readonly("rows", &Plan::rows)
      .def_property_readonly("rows_pad", &Plan::rows_pad)
      .def_property_readonly("dim", &Plan::dim)
      .def_property_readonly("dim_k", &Plan::dim_k)
      .def_property_readonly("ld_k", &Plan::ld_k)
      .def_property_readonly("ld_t", &Plan::ld_t)
      .def_property_readonly("dim_n", &Plan::dim_n)
      .def_property_readonly("world", &Plan::world)
      .def_property_readonly("rank", &Plan::rank)
      .def_property_readonly("row_tiles", &Plan::row_tiles)
      .def_property_readonly("col_tiles", &Plan::col_tiles)
      .def_property_readonly("temperature", &Plan::temperature)
      .def_property_readonly("compute_dtype", &Plan::compute_dtype)
      .def_property_readonly("backward_dtype", &Plan::backward_dtype_name)
      .def_property_readonly("ld_k8", [](const Plan& p) { return p.g.ld_k8; })
      .def_readonly("n_fwd_tiles", &Plan::n_fwd)
      .def_readonly("n_own_tiles", &Plan::n_own)
      .def_readonly("n_dz_tiles", &Plan::n_dz)
      .def_readonly("small", &Plan::small)
      .def_readonly("fwd_tiles", &Plan::fwd_tiles)
      .def_readonly("dz_tiles", &Plan::dz_tiles);
  // one RCCL communicator per (process group, device), shared by the engines of every shape
  py::class_<ntxent::RcclComm, std::shared_ptr<ntxent::RcclComm>>(m, "RcclCommunicator")
      .def(py::init([](int rank, int world, const py::bytes& uid, int device) {
             return std::make_shared<ntxent::RcclComm>(rank, world, std::string(uid), device);
           }),
           py::arg("rank"), py::arg("world"), py::arg("uid"), py::arg("device"))
      .def_property_readonly("rank", &ntxent::RcclComm::rank)
      .def_property_readonly("world", &ntxent::RcclComm::world)
      .def("check", &ntxent::RcclComm::check)
      .def("abort", &ntxent::RcclComm::abort);
  py::class_<NativeEngine>(m, "NativeEngine")
      .def(py::init<int, int, double, const std::string&, const std::string&, const std::string&, int, int,
                    const std::string&, int, bool, int, std::shared_ptr<ntxent::RcclComm>, bool>(),
           py::arg("rows"), py::arg("dim"), py::arg("temperature"), py::arg("input") = "bf16",
           py::arg("compute") = "auto", py::arg("negatives") = "symmetric", py::arg("rank") = 0, py::arg("world") = 1,
           py::arg("uid") = std::string(), py::arg("device") = 0, py::arg("keep_cos") = true,
           py::arg("comm_reserve_cus") = 8, py::arg("comm") = py::none(), py::arg("temperature_grad") = false)
      .def("forward", &NativeEngine::forward, py::arg("h"))
      .def("backward", &NativeEngine::backward, py::arg("grad_out") = py::none())
      .def("loss_tensor", &NativeEngine::loss_tensor)
      .def("step", &NativeEngine::step, py::arg("h"))
      .def("capture", &NativeEngine::capture, py::arg("h"))
      .def("replay", &NativeEngine::replay)
      .def("set_temperature", &NativeEngine::set_temperature, py::arg("temperature"))
      .def("temperature_grad", &NativeEngine::temperature_grad)
      .def("positive_rank", &NativeEngine::positive_rank, py::arg("h"))
      .def_property_readonly("temperature", &NativeEngine::temperature)
      .def_property_readonly("captured", &NativeEngine::captured)
      .def_property_readonly("device_bytes", &NativeEngine::device_bytes)
      .def_property_readonly("symmetric", &NativeEngine::symmetric)
      .def_property_readonly("small", &NativeEngine::small)
      .def_property_readonly("rank", &NativeEngine::rank)
      .def_property_readonly("world", &NativeEngine::world);
  m.def("rccl_unique_id", []() { return py::bytes(ntxent::RcclComm::unique_id()); });
  m.def("get_plan", &get_plan, py::arg("rows"), py::arg("dim"), py::arg("world"), py::arg("rank"),
        py::arg("temperature"), py::arg("compute"), py::arg("device"));
  m.def("choose_compute", [](const std::string& in_dtype, bool mp, const std::string& ov) {
    at::ScalarType t = in_dtype == "float32" ? at::kFloat : (in_dtype == "float16" ? at::kHalf : at::kBFloat16);
    return std::string(ntxent::dtype_name(choose_compute(t, mp, ov)));
  });
  m.def("prep", &prep, py::arg("h"), py::arg("plan"), py::arg("zq_out") = py::none(), py::arg("zq8_out") = py::none());
  m.def("transpose", &transpose, py::arg("zq"), py::arg("plan"), py::arg("zqt_out") = py::none());
  m.def("pos_rank", &pos_rank, py::arg("zq"), py::arg("plan"),
        "Stage op: (rank, pos_cos, hard_neg_cos) of prep's unit rows zq for a world-1 plan.");
  m.def("positive_rank", &positive_rank, py::arg("h"), py::arg("compute") = "auto",
        py::arg("use_mixed_precision") = false,
        "(rank, pos_cos, hard_neg_cos) of stacked views h = [h1; h2] on the current stream: rank[i] counts the "
        "negatives whose cosine is strictly larger than the positive's. compute: auto|fp32|fp16|bf16|fp8, "
        "resolved as for the loss; fp8 computes in fp16.");
  m.def("fwd_stats_range", &fwd_stats_range, py::arg("zq_local"), py::arg("zq_all"), py::arg("plan"), py::arg("part"),
        py::arg("sc"), py::arg("first"), py::arg("count"), py::arg("reserve_cus") = 0);
  m.def("fwd_stats", [](const at::Tensor& zl, const at::Tensor& za, const Plan& P, bool keep) {
    return fwd_stats(zl, za, P, keep, true);
  }, py::arg("zq_local"), py::arg("zq_all"), py::arg("plan"), py::arg("keep_cos"));
  m.def("lse", &lse, py::arg("part"), py::arg("ypos"), py::arg("lse2_all"), py::arg("cpos"), py::arg("plan"),
        py::arg("zq") = py::none(), py::arg("zqt") = py::none());
  m.def("coef", &coef, py::arg("sbuf"), py::arg("lse2_all"), py::arg("cpos"), py::arg("plan"));
  m.def("coef_gemm", &coef_gemm);
  m.def("dz", &dz);
  m.def("set_fp8_backward", &ntxent::set_fp8_backward, py::arg("on"));
  m.def("set_raw_forward", &ntxent::set_raw_forward, py::arg("on"));
  m.def("raw_forward_enabled", &ntxent::raw_forward_enabled);
  m.def("set_lse_fold", &ntxent::set_lse_fold, py::arg("on"));
  m.def("lse_fold_enabled", &ntxent::lse_fold_enabled);
  m.def("set_half_c", &ntxent::set_half_c, py::arg("on"));
  m.def("half_c_enabled", &ntxent::half_c_enabled);
  m.def("set_dot_fold", &ntxent::set_dot_fold, py::arg("on"));
  m.def("dot_fold_enabled", &ntxent::dot_fold_enabled);
  m.def("set_dot_fold_spin", &ntxent::set_dot_fold_spin, py::arg("polls"));
  m.def("dot_fold_spin", &ntxent::dot_fold_spin);
  m.def("fp8_backward_enabled", &ntxent::fp8_backward_enabled);
  m.def("fwd_splitk_pieces", &ntxent::fwd_splitk_pieces, py::arg("ntiles"), py::arg("nk"), py::arg("cus"),
        py::arg("diag_tail"));
  m.def("fwd_diag_remainder", &ntxent::fwd_diag_remainder, py::arg("ntiles"), py::arg("nk"), py::arg("cus"),
        py::arg("diag_tail"), py::arg("f8") = false);
  m.def("norm_bwd", &norm_bwd, py::arg("slabs"), py::arg("h"), py::arg("inv"), py::arg("grad_out"), py::arg("plan"));
  m.def("fwd_stats_tiles", &fwd_stats_tiles, py::arg("zq_local"), py::arg("zq_chunk"), py::arg("b_tile0"),
        py::arg("tiles"), py::arg("plan"), py::arg("part"), py::arg("reserve_cus") = 0);
  m.def("coef_gemm_tiles", &coef_gemm_tiles, py::arg("zq_local"), py::arg("zq_chunk"), py::arg("b_tile0"),
        py::arg("tiles"), py::arg("lse2_all"), py::arg("cpos"), py::arg("plan"), py::arg("c_ld"), py::arg("c_tile0"),
        py::arg("reserve_cus") = 0);
  m.def("dz_block", &dz_block, py::arg("cbuf_block"), py::arg("zqt_chunk"), py::arg("plan"), py::arg("reserve_cus") = 0);
  m.def("dz_view", &dz_view, py::arg("abuf"), py::arg("a_tile0"), py::arg("a_panel_tiles"), py::arg("bbuf"),
        py::arg("b_block0"), py::arg("b_col0"), py::arg("k_tiles"), py::arg("m0"), py::arg("m1"), py::arg("out"),
        py::arg("accum"), py::arg("plan"), py::arg("reserve_cus") = 0);
  // the symmetric step (sym_step.h): one cached object per shape, its phases over a tensor bundle
  {
    const auto plan = py::arg("plan"), bufs = py::arg("bufs");
    const auto reserve = py::arg("reserve_cus") = 0;
    py::class_<SymStep, std::shared_ptr<SymStep>>(m, "SymStep")
        .def_property_readonly("plan", [](const SymStep& S) { return sym_plan_dict(S.sp); })
        .def("prep", sym_phase<>([](const SymStep& S, const Plan& P, SymBundle& x, hipStream_t s) {
          ntxent::sym_prep(S.sp, P.g, x.in, x.b, s);
        }), plan, bufs)
        .def("fwd_tiles_range", sym_phase<int, int, int>([](const SymStep& S, const Plan& P, SymBundle& x, hipStream_t s,
                                                            int first, int count, int reserve_cus) {
          ntxent::sym_fwd_tiles(S.sp, P.g, P.comp, x.b, first, count, gemm_ws(x.like, count, P, reserve_cus), s);
        }), plan, bufs, py::arg("first"), py::arg("count"), reserve)
        .def("lse", sym_phase<>([](const SymStep& S, const Plan& P, SymBundle& x, hipStream_t s) {
          x.b.block_loss = static_cast<float*>(device_scratch(x.like, (size_t)ntxent::lse_scratch_floats(P.g) * 4, 1).data_ptr());
          ntxent::sym_lse(S.sp, P.g, x.b, s);
        }), plan, bufs)
        .def("transpose_partners", sym_phase<>([](const SymStep& S, const Plan& P, SymBundle& x, hipStream_t s) {
          ntxent::sym_transpose_partners(S.sp, P.g, x.b, s);
        }), plan, bufs)
        .def("coef", sym_phase<>([](const SymStep& S, const Plan& P, SymBundle& x, hipStream_t s) {
          ntxent::sym_coef(S.sp, P.g, x.b, s);
        }), plan, bufs)
        .def("partner_grads", sym_phase<int>([](const SymStep& S, const Plan& P, SymBundle& x, hipStream_t s, int reserve_cus) {
          ntxent::sym_partner_grads(S.sp, P.g, x.b, gemm_ws(x.like, P.n_dz, P, reserve_cus), s);
        }), plan, bufs, reserve)
        .def("own_grads", sym_phase<int>([](const SymStep& S, const Plan& P, SymBundle& x, hipStream_t s, int reserve_cus) {
          ntxent::sym_own_grads(S.sp, P.g, x.b, gemm_ws(x.like, P.n_dz, P, reserve_cus), s);
        }), plan, bufs, reserve)
        .def("norm_bwd", sym_phase<>([](const SymStep& S, const Plan& P, SymBundle& x, hipStream_t s) {
          NTXENT_CHECK(x.own_bytes == S.sp.bytes.own, "own: must be the fp32 slab (fp32 plans: the stack with the received slabs)");
          ntxent::sym_norm_bwd(S.sp, P.g, x.in, x.b, s);
        }), plan, bufs);
  }
  m.def("sym_step", &sym_step, py::arg("plan"));
  m.def("fused_forward", &fused_forward, py::arg("h"), py::arg("T"), py::arg("compute") = "auto",
        py::arg("keep_cos") = true);
  m.def("fused_backward", &fused_backward);
  m.def("fused_backward_tau", &fused_backward_tau);
  m.def("xview_forward", &xview_forward, py::arg("h"), py::arg("T"), py::arg("compute") = "auto");
  m.def("xview_backward", &xview_backward);
  m.def("xview_backward_tau", &xview_backward_tau);
  m.def("xview_sigmoid_forward", &xview_sigmoid_forward, py::arg("h"), py::arg("T"), py::arg("bias"),
        py::arg("compute") = "auto");
  m.def("xview_sigmoid_backward", &xview_sigmoid_backward);
  m.def("xview_dist_part_slots", [](const Plan& P) { return (long)(xview_part_bytes(P.g) / 8 / P.g.rows_pad); });
  m.def("xview_dist_coef_bytes", [](const Plan& P) { return (long)xview_coef_bytes(P.bwd(), P.g); });
  m.def("xview_dist_fwd", &xview_dist_fwd, py::arg("zq_all"), py::arg("plan"), py::arg("part"), py::arg("ypos"),
        py::arg("q_lo"), py::arg("q_hi"), py::arg("q_skip") = -1);
  m.def("xview_dist_lse", &xview_dist_lse, py::arg("part"), py::arg("ypos"), py::arg("lse2_all"), py::arg("cpos"),
        py::arg("plan"));
  m.def("xview_dist_backward", &xview_dist_backward, py::arg("h"), py::arg("zq_all"), py::arg("inv"),
        py::arg("lse2_all"), py::arg("cpos"), py::arg("grad_out"), py::arg("plan"));
  m.def("xview_sigmoid_dist_tiles", [](const Plan& P) { return (long)(xview_sigmoid_scratch_bytes(P.g) / 8); });
  m.def("xview_sigmoid_dist_fwd", &xview_sigmoid_dist_fwd, py::arg("zq_all"), py::arg("plan"), py::arg("lpart"),
        py::arg("h"), py::arg("inv"), py::arg("bias"), py::arg("q_lo"), py::arg("q_hi"), py::arg("q_skip") = -1);
  m.def("xview_sigmoid_dist_loss", &xview_sigmoid_dist_loss, py::arg("lpart"), py::arg("plan"));
  m.def("xview_sigmoid_dist_backward", &xview_sigmoid_dist_backward, py::arg("h"), py::arg("zq_all"), py::arg("inv"),
        py::arg("grad_out"), py::arg("plan"), py::arg("bias"), py::arg("want_tau"), py::arg("want_bias"));
  // block form (exchange="ring"): the caller's buffers, in bytes / elements
  m.def("xview_sigmoid_block_sizes", [](const Plan& P) {
    py::dict d;
    d["coef_bytes"] = (long)xview_block_coef_bytes(P.comp, P.g);
    d["zt_bytes"] = (long)xview_block_zt_bytes(P.comp, P.g);
    d["bias_part"] = (long)(xview_sigmoid_bias_part_bytes(P.g) / 4);
    d["dz"] = (long)(xview_dz_bytes(P.g) / 4);
    d["gather_coef_bytes"] = (long)xview_coef_bytes(P.comp, P.g);
    d["gather_zt_bytes"] = (long)xview_zt_bytes(P.comp, P.g);
    return d;
  });
  m.def("xview_sigmoid_pos_cos", &xview_sigmoid_pos_cos, py::arg("h"), py::arg("inv"), py::arg("plan"));
  m.def("xview_sigmoid_block_fwd", &xview_sigmoid_block_fwd, py::arg("zq"), py::arg("rows_q"), py::arg("q"),
        py::arg("plan"), py::arg("lpart"), py::arg("h"), py::arg("inv"), py::arg("bias"));
  m.def("xview_sigmoid_block_backward", &xview_sigmoid_block_backward, py::arg("zq"), py::arg("rows_q"), py::arg("q"),
        py::arg("plan"), py::arg("bias"), py::arg("coef"), py::arg("zt"), py::arg("bias_part"), py::arg("dz"),
        py::arg("pos_cos"), py::arg("first"));
  m.def("xview_sigmoid_ring_finish", &xview_sigmoid_ring_finish, py::arg("h"), py::arg("inv"), py::arg("grad_out"),
        py::arg("dz"), py::arg("bias_part"), py::arg("plan"), py::arg("want_tau"), py::arg("want_bias"));
  m.def("tile_list_uploads", []() { return g_tile_uploads.load(); });
  m.def("set_small_path", &ntxent::set_small_path, py::arg("on"));
  m.def("small_path_enabled", &ntxent::small_path_enabled);
  m.def("set_small_splits", &ntxent::set_small_splits, py::arg("n"));
  m.def("set_small_fuse_rows", &ntxent::set_small_fuse_rows, py::arg("rows"));
  m.def("small_fwd_fused", [](const Plan& P) { return ntxent::small_fwd_fused(P.g); });
  // reference API names and kwargs
  m.def("forward", &forward_op, py::arg("z"), py::arg("T"), py::arg("use_mixed_precision") = false);
  m.def("forward_with_stats", &forward_with_stats, py::arg("z"), py::arg("T"), py::arg("use_mixed_precision") = false);
  m.def("backward", &backward_op, py::arg("z"), py::arg("softmax"), py::arg("grad_out"), py::arg("T"),
        py::arg("use_mixed_precision") = false, py::arg("want_grad_logits") = false);
  m.def("check_tensor_core_support", &check_tensor_core_support);
  m.def("check_matrix_core_support", &check_tensor_core_support);
  m.def("get_optimal_block_size", &ntxent::get_optimal_block_size);
  m.def("device_info", [](int dev) {
    const auto& d = ntxent::device_info(dev);
    py::dict r;
    r["device"] = d.device;
    r["num_cus"] = d.num_cus;
    r["lds_per_block"] = d.lds_per_block;
    r["warp_size"] = d.warp_size;
    r["arch"] = d.arch;
    r["is_gfx950"] = d.is_gfx950;
    return r;
  });
  // host-only planning helpers (no device needed: unit-tested on CPU)
  m.def("geometry", [](int rows, int dim, int world, int rank, double T) {
    const auto g = ntxent::make_geometry(rows, dim, world, rank, (float)T);
    py::dict r;
    r["rows"] = g.rows; r["rows_pad"] = g.rows_pad; r["dim"] = g.dim; r["dim_k"] = g.dim_k;
    r["dim_n"] = g.dim_n; r["ld_k"] = g.ld_k; r["ld_t"] = g.ld_t; r["world"] = g.world;
    r["rank"] = g.rank; r["row_tiles"] = g.row_tiles; r["col_tiles"] = g.col_tiles;
    r["global_rows"] = g.global_rows;
    return r;
  }, py::arg("rows"), py::arg("dim"), py::arg("world") = 1, py::arg("rank") = 0, py::arg("T") = 0.07);
  auto tiles_to_list = [](const std::vector<int4>& v) {
    py::list l;
    for (const auto& t : v) l.append(py::make_tuple(t.x, t.y, t.z));
    return l;
  };
  m.def("fwd_tile_list", [tiles_to_list](int rows, int dim, int world, int rank) {
    return tiles_to_list(ntxent::build_fwd_tiles(ntxent::make_geometry(rows, dim, world, rank, 0.07f)));
  }, py::arg("rows"), py::arg("dim"), py::arg("world") = 1, py::arg("rank") = 0);
  m.def("dz_tile_list", [tiles_to_list](int rows, int dim, int world, int rank) {
    return tiles_to_list(ntxent::build_dz_tiles(ntxent::make_geometry(rows, dim, world, rank, 0.07f)));
  }, py::arg("rows"), py::arg("dim"), py::arg("world") = 1, py::arg("rank") = 0);
  m.def("sym_fwd_tile_list", [tiles_to_list](int rows, int dim, int world, int rank) {
    const auto g = ntxent::make_geometry(rows, dim, world, rank, 0.07f);
    const auto p = ntxent::make_sym_plan(g, ntxent::DType::F16, false);
    return tiles_to_list(ntxent::build_sym_fwd_tiles(g, p.jobs, p.nchunks));
  }, py::arg("rows"), py::arg("dim"), py::arg("world"), py::arg("rank"));
  // the schedule of the symmetric step (sym_step.h) of one rank
  m.def("sym_plan", [](int rows, int dim, int world, int rank, const std::string& compute) {
    const ntxent::DType comp = parse_dtype_name(compute);
    return sym_plan_dict(ntxent::make_sym_plan(ntxent::make_geometry(rows, dim, world, rank, 0.07f),
                                               ntxent::backward_dtype(comp), comp == ntxent::DType::FP8));
  }, py::arg("rows"), py::arg("dim"), py::arg("world"), py::arg("rank"), py::arg("compute") = "fp16");
  m.def("schedule", [](int ntiles, int nk, int num_cus) {
    const auto s = ntxent::make_schedule(ntiles, nk, num_cus);
    py::dict r;
    r["grid"] = s.grid; r["nk"] = s.nk; r["dp_tiles"] = s.dp_tiles; r["sk_tiles"] = s.sk_tiles;
    r["ipb"] = s.ipb;
    return r;
  }, py::arg("ntiles"), py::arg("nk"), py::arg("num_cus"));
  m.def("gemm_workspace_bytes", &ntxent::gemm_workspace_bytes);
  // the decisions of the one-GPU step (step.h), as the autograd op and the Engine resolve them
  m.def("step_plan", [](int rows, int dim, const std::string& input, const std::string& compute, bool keep_cos,
                        int num_cus) {
    const ntxent::DType comp = parse_dtype_name(compute);
    const auto p = ntxent::resolve_step_plan(ntxent::make_geometry(rows, dim, 1, 0, 0.07f), parse_dtype_name(input),
                                             comp, keep_cos || comp == ntxent::DType::FP8, num_cus);
    py::dict r;
    r["small"] = p.small; r["small_fwd_fused"] = p.small_fwd_fused; r["small_splits"] = p.small_splits;
    r["f8"] = p.f8; r["q8"] = p.q8; r["raw"] = p.raw; r["fuse"] = p.fuse; r["half_c"] = p.half_c;
    r["dfold"] = p.dfold; r["keep_cos"] = p.keep_cos; r["bwd"] = ntxent::dtype_name(p.bwd);
    r["n_fwd"] = p.n_fwd; r["n_own"] = p.n_own; r["n_dz"] = p.n_dz;
    r["forward_mfma"] = ntxent::dtype_name(p.fwd_mfma); r["backward_mfma"] = ntxent::dtype_name(p.bwd_mfma);
    return r;
  }, py::arg("rows"), py::arg("dim"), py::arg("input"), py::arg("compute"), py::arg("keep_cos") = true,
     py::arg("num_cus") = 256);
  // The NT-Xent pair rule of the kernels (kernels/pair_mask.h) on the host, for
  // tests/test_pair_mask_cpu.py: thin wrappers, the loops over a whole square included.
  m.def("pair_partner", [](int i, int n_half) { return ntxent::pair::partner(i, n_half); });
  m.def("pair_negative_matrix", [](int R, int n_half, int n) {  // [n][n]: is_negative(i, j)
    auto out = at::empty({n, n}, at::kBool);
    bool* o = out.data_ptr<bool>();
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) o[(size_t)i * n + j] = ntxent::pair::is_negative(i, j, R, n_half);
    return out;
  });
  // [n][n]: TileMask::drop of every element, each through the tile x tile tile that holds it
  m.def("pair_drop_matrix", [](int R, int n_half, int n, int tile, bool diag) {
    auto out = at::empty({n, n}, at::kBool);
    bool* o = out.data_ptr<bool>();
    for (int r0 = 0; r0 < n; r0 += tile)
      for (int c0 = 0; c0 < n; c0 += tile) {
        const ntxent::pair::TileMask tm(R, n_half, r0, c0);
        for (int tr = 0; tr < tile && r0 + tr < n; ++tr)
          for (int tc = 0; tc < tile && c0 + tc < n; ++tc) o[(size_t)(r0 + tr) * n + c0 + tc] = tm.drop(tr, tc, diag);
      }
    return out;
  }, py::arg("R"), py::arg("n_half"), py::arg("n"), py::arg("tile"), py::arg("diag") = true);
  m.def("pair_window_plain", &ntxent::pair::window_plain, py::arg("r_lo"), py::arg("nr"), py::arg("c_lo"), py::arg("nc"),
        py::arg("own0"), py::arg("R"), py::arg("n_half"), py::arg("c_local"));
  m.def("pair_tile_near", [](int R, int n_half, int r0, int c0) { return ntxent::pair::TileMask(R, n_half, r0, c0).near(); });
  m.def("pair_fragment_near", [](int R, int n_half, int r0, int c0, int off) {
    return ntxent::pair::TileMask(R, n_half, r0, c0).fragment_near(off);
  });
  m.attr("TILE") = ntxent::kTile;
  m.attr("K_STEP_BYTES") = ntxent::kKStepBytes;
}
