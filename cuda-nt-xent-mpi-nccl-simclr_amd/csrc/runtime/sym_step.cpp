// The symmetric data-parallel step (see include/ntxent/sym_step.h): the block assignment, the
// schedule every driver walks, the buffer sizes and the compute phases.
// No reference counterpart (the reference has no multi-GPU code).
#include "ntxent/sym_step.h"

#include <algorithm>

#include "ntxent/trace.h"

namespace ntxent {

// ---- the assignment ---------------------------------------------------------------------
// The W(W-1)/2 off-diagonal blocks are split evenly: rank r computes the blocks (r, r+1), ...,
// (r, r+(W-1)/2) (mod W) in full and, for even W, its share of the block (r, r + W/2), which the
// pair splits by the lower rank's row tiles (lower rank: its tiles [0, h); upper rank: all its
// tiles x the lower rank's [h, rt)).
std::vector<SymJob> sym_jobs(int world, int rank, int row_tiles) {
  std::vector<SymJob> jobs;
  const int W = world, r = rank, rt = row_tiles;
  for (int d = 1; d <= (W - 1) / 2; ++d) jobs.push_back(SymJob{(r + d) % W, 0, rt, 0, rt});
  if (W % 2 == 0 && W > 1) {
    const int q = (r + W / 2) % W, h = (rt + 1) / 2;
    const SymJob j = r < q ? SymJob{q, 0, h, 0, rt} : SymJob{q, 0, rt, h, rt};
    if (j.m0 < j.m1 && j.k0 < j.k1) jobs.push_back(j);
  }
  return jobs;
}

std::vector<SymJob> sym_incoming(int world, int rank, int row_tiles) {
  std::vector<SymJob> out;
  for (int p = 0; p < world; ++p) {
    if (p == rank) continue;
    for (const SymJob& j : sym_jobs(world, p, row_tiles))
      if (j.q == rank) out.push_back(SymJob{p, j.m0, j.m1, j.k0, j.k1});
  }
  return out;
}

// Forward rows travel in up to 4 chunks (8 MiB each at B = 4096, d = 2048): the cross tiles of
// chunk c start while chunk c + 1 is on the wire.
int sym_num_chunks(int row_tiles) { return std::max(1, std::min(4, row_tiles)); }

std::pair<int, int> sym_chunk_bounds(int row_tiles, int c, int nchunks) {
  return {(int)((long long)row_tiles * c / nchunks), (int)((long long)row_tiles * (c + 1) / nchunks)};
}

int sym_c_ld(const Geometry& g) { return std::min(g.world, g.world / 2 + 1) * g.row_tiles; }

namespace {

int mod(int a, int n) { return (a % n + n) % n; }

// the part of a job's partner row tiles [k0, k1) inside chunk c (empty: first >= second)
std::pair<int, int> in_chunk(const SymJob& j, int rt, int c, int nch) {
  const auto b = sym_chunk_bounds(rt, c, nch);
  return {std::max(j.k0, b.first), std::min(j.k1, b.second)};
}

// Appends a dZ call; its (m0, m1) tile list (row tiles x every dim_n tile) is shared by equal ranges.
struct DzCalls {
  const Geometry& g;
  SymPlan& p;
  std::vector<std::pair<std::pair<int, int>, size_t>> ranges;
  void add(std::vector<SymDzCall>& to, bool mirror, long long a_tile0, long long a_panel, int b_block0, long long b_col0,
           int k_tiles, int m0, int m1, int out, bool accum) {
    if (m1 <= m0 || k_tiles == 0) return;
    const long long kcols = (long long)k_tiles * kTile;
    long long kblk = kcols;
    if (b_col0 + kcols > g.rows_pad) {
      NTXENT_CHECK(b_col0 == 0 && kcols % g.rows_pad == 0, "symmetric step: multi-block K must cover whole blocks");
      kblk = g.rows_pad;
    }
    NTXENT_CHECK(b_block0 >= 0 && b_block0 + (kcols + kblk - 1) / kblk <= g.world, "symmetric step: B view out of bounds");
    NTXENT_CHECK(!(out >= 0 && p.contrib_f16 && accum), "symmetric step: fp16 output cannot accumulate");
    size_t off = 0;
    bool hit = false;
    for (const auto& r : ranges)
      if (r.first == std::make_pair(m0, m1)) { off = r.second; hit = true; }
    if (!hit) {
      off = p.dz_rows.size();
      for (int ti = m0; ti < m1; ++ti)
        for (int n = 0; n < g.dim_n / kTile; ++n) p.dz_rows.push_back(make_int4(ti, n, 0, 0));
      ranges.push_back({{m0, m1}, off});
    }
    to.push_back(SymDzCall{mirror, a_tile0, a_panel, b_block0, b_col0, kblk, k_tiles, m0, m1, out, accum, off});
  }
};

}  // namespace

SymPlan make_sym_plan(const Geometry& g, DType bwd, bool f8) {
  SymPlan p;
  const int W = p.world = g.world, r = p.rank = g.rank, rt = p.row_tiles = g.row_tiles;
  p.bwd = bwd;
  p.f8 = f8;
  p.contrib_f16 = bwd != DType::F32;
  p.jobs = sym_jobs(W, r, rt);
  p.incoming = sym_incoming(W, r, rt);
  p.nchunks = sym_num_chunks(rt);
  p.c_ld = sym_c_ld(g);
  p.n_own = count_own_fwd_tiles(g);
  auto full = [rt](const SymJob& j) { return j.m0 == 0 && j.m1 == rt && j.k0 == 0 && j.k1 == rt; };
  for (const SymJob& j : p.jobs) p.nfull += full(j) ? 1 : 0;
  for (int i = 0; i < p.nfull; ++i) NTXENT_CHECK(full(p.jobs[i]), "symmetric step: full blocks must precede the split block");
  p.split = (int)p.jobs.size() > p.nfull;
  NTXENT_CHECK((int)p.jobs.size() <= p.nfull + 1, "symmetric step: more than one split block");

  // forward: each chunk's cross-tile segment (build_sym_fwd_tiles order) and its row exchange
  int first = p.n_own;
  p.rows.resize(p.nchunks);
  for (int c = 0; c < p.nchunks; ++c) {
    int n = 0;
    for (const SymJob& j : p.jobs) {
      const auto a = in_chunk(j, rt, c, p.nchunks);
      n += (j.m1 - j.m0) * std::max(0, a.second - a.first);
    }
    p.segs.push_back({first, n});
    first += n;
    for (const SymJob& i : p.incoming) {  // i.q uses my row tiles [k0, k1)
      const auto a = in_chunk(i, rt, c, p.nchunks);
      if (a.first < a.second) p.rows[c].push_back({true, i.q, 0, 0, a.first, a.second, -1});
    }
    for (const SymJob& j : p.jobs) {  // I use q's row tiles [k0, k1)
      const auto a = in_chunk(j, rt, c, p.nchunks);
      if (a.first < a.second) p.rows[c].push_back({false, j.q, 0, 0, a.first, a.second, -1});
    }
  }
  p.n_fwd = first;
  if (f8) {  // the backward runs on the fp16 rows
    for (const SymJob& i : p.incoming) p.rows_f16.push_back({true, i.q, 0, 0, i.k0, i.k1, -1});
    for (const SymJob& j : p.jobs) p.rows_f16.push_back({false, j.q, 0, 0, j.k0, j.k1, -1});
  }
  // column partials of the cross tiles -> their rows' owners: rank q's part slots [r * rt + m] for
  // its rows [k0, k1), one run per row tile m, Rpad apart. A whole-block job (k0 = 0, k1 = rt) has
  // its runs back to back; the k-split block's runs can be packed (one message per partner
  // instead of one per row tile).
  size_t xs = 0, xr = 0;
  auto packed = [rt](const SymJob& j, size_t& off) {
    if (j.k1 - j.k0 == rt) return (long long)-1;
    const long long at = (long long)off;
    off += (size_t)(j.m1 - j.m0) * (j.k1 - j.k0) * kTile;
    return at;
  };
  for (const SymJob& j : p.jobs) p.col_partials.push_back({true, j.q, j.q * rt + j.m0, j.q * rt + j.m1, j.k0, j.k1, packed(j, xs)});
  for (const SymJob& i : p.incoming)
    p.col_partials.push_back({false, i.q, i.q * rt + i.m0, i.q * rt + i.m1, i.k0, i.k1, packed(i, xr)});

  // backward. mbuf holds the partners' mirrored blocks [slot][rt][rt] with slot = (q - r - 1) mod W
  // (job order); cbuf is compact, column block r + d at column slots [d * rt, (d + 1) * rt).
  DzCalls dz{g, p, {}};
  // the partners' contributions C_{q,r} Z_r: the full blocks in ONE stacked GEMM (a tall A of
  // nfull x rt row panels, slabs 0 .. nfull-1), then the split block's rows into slab nfull
  if (p.nfull > 0) dz.add(p.partner_dz, true, 0, rt, r, 0, rt, 0, p.nfull * rt, 0, false);
  if (p.split) {
    const SymJob& s = p.jobs.back();
    dz.add(p.partner_dz, true, (long long)mod(s.q - r - 1, W) * rt * rt + s.m0, rt, r, (long long)s.m0 * kTile, s.m1 - s.m0,
           s.k0, s.k1, p.nfull, false);
  }
  // own contributions: C_{r,r} Z_r + the full blocks (consecutive rank blocks r .. r+nfull, two
  // GEMMs if they wrap) + the split block's rows
  const int nb = 1 + p.nfull, head = std::min(nb, W - r);
  dz.add(p.own_dz, false, 0, p.c_ld, r, 0, head * rt, 0, rt, -1, false);
  if (nb > head) dz.add(p.own_dz, false, (long long)head * rt, p.c_ld, 0, 0, (nb - head) * rt, 0, rt, -1, true);
  if (p.split) {
    const SymJob& s = p.jobs.back();
    dz.add(p.own_dz, false, (long long)mod(s.q - r, W) * rt + s.k0, p.c_ld, s.q, (long long)s.k0 * kTile, s.k1 - s.k0, s.m0, s.m1,
           -1, true);
  }
  for (size_t i = 0; i < p.jobs.size(); ++i) p.contribs.push_back({true, p.jobs[i].q, (int)i, (int)i + 1, p.jobs[i].k0, p.jobs[i].k1, -1});
  for (size_t i = 0; i < p.incoming.size(); ++i)
    p.contribs.push_back({false, p.incoming[i].q, (int)i, (int)i + 1, p.incoming[i].k0, p.incoming[i].k1, -1});

  const size_t cs = dtype_size(bwd), tile = (size_t)kTileElems * cs;
  SymBufferBytes& b = p.bytes;
  b.sbuf = (size_t)p.n_fwd * tile;
  b.cbuf = (size_t)rt * p.c_ld * tile;
  b.mbuf = (size_t)std::max(1, W / 2) * rt * rt * tile;
  b.part_x = (size_t)g.col_tiles * g.rows_pad * sizeof(float2);
  b.slab = (size_t)g.rows_pad * g.dim_n * (p.contrib_f16 ? 2 : 4);
  b.contrib = p.jobs.size() * b.slab;
  b.recv = p.contrib_f16 ? p.incoming.size() * b.slab : 0;
  b.own = (size_t)g.rows_pad * g.dim_n * 4 * (p.contrib_f16 ? 1 : 1 + p.incoming.size());
  b.xsend = xs * sizeof(float2);
  b.xrecv = xr * sizeof(float2);
  b.dz_rows = p.dz_rows.size() * sizeof(int4);
  return p;
}

// ---- the phases -------------------------------------------------------------------------
namespace {

size_t cs_of(const SymPlan& p) { return dtype_size(p.bwd); }
char* rows_of(const SymPlan& p, const Geometry& g, void* zq_all, int q) {
  return static_cast<char*>(zq_all) + (size_t)q * g.rows_pad * g.ld_k * cs_of(p);
}
char* zqt_of(const SymPlan& p, const Geometry& g, void* zqt_all, int q) {
  return static_cast<char*>(zqt_all) + (size_t)q * g.dim_n * g.ld_t * cs_of(p);
}

// The one place a dZ call record becomes pointers.
void dz_call(const SymPlan& p, const Geometry& g, const SymDzCall& c, const SymBuffers& b, const GemmWorkspace& ws,
             hipStream_t s) {
  const size_t cs = cs_of(p);
  const long long blk = (long long)g.dim_n * g.ld_t;
  NTXENT_CHECK((c.mirror ? b.mbuf : b.cbuf) && b.zqt_all && (c.out < 0 ? (void*)b.own : b.contrib) && b.dz_rows,
               "symmetric step: dZ buffer missing");
  const char* a = static_cast<const char*>(c.mirror ? b.mbuf : b.cbuf) + (size_t)c.a_tile0 * kTileElems * cs;
  const char* bb = static_cast<const char*>(b.zqt_all) + ((size_t)c.b_block0 * blk + c.b_col0) * cs;
  void* out = c.out < 0 ? static_cast<void*>(b.own) : static_cast<char*>(b.contrib) + (size_t)c.out * p.bytes.slab;
  launch_dz_view(p.bwd, a, c.a_panel_tiles, bb, c.b_kblk_cols, blk, c.k_tiles, b.dz_rows + c.rows_off,
                 (c.m1 - c.m0) * (g.dim_n / kTile), out, c.accum, ws, g, s, c.out >= 0 && p.contrib_f16);
}

}  // namespace

void sym_prep(const SymPlan& p, const Geometry& g, DType in, const SymBuffers& b, hipStream_t s) {
  NTXENT_TRACE("ntxent.prep");
  fault_point("prep");
  NTXENT_CHECK(b.h && b.zq_all && b.zqt_all && b.inv && b.ypos && (!p.f8 || b.zq8_all), "symmetric step: prep buffer missing");
  char* zq = rows_of(p, g, b.zq_all, p.rank);
  launch_prep(in, p.bwd, b.h, zq, b.inv, b.ypos, g, s,
              p.f8 ? static_cast<char*>(b.zq8_all) + (size_t)p.rank * g.rows_pad * g.ld_k8 : nullptr);
  launch_transpose(p.bwd, zq, zqt_of(p, g, b.zqt_all, p.rank), g, s);  // own B operand of the backward
}

void sym_fwd_tiles(const SymPlan& p, const Geometry& g, DType comp, const SymBuffers& b, int first, int count,
                   const GemmWorkspace& ws, hipStream_t s) {
  NTXENT_CHECK(first >= 0 && count >= 0 && first + count <= p.n_fwd, "symmetric step: tile range out of bounds");
  if (count == 0) return;
  const bool own = first + count == p.n_own;
  NTXENT_TRACE(own ? "ntxent.fwd_gemm.own" : "ntxent.fwd_gemm.cross");
  if (own) fault_point("fwd");
  char* op_all = static_cast<char*>(p.f8 ? b.zq8_all : b.zq_all);
  NTXENT_CHECK(op_all && b.fwd_tiles && b.part && b.part_x, "symmetric step: forward buffer missing");
  const size_t op_row = p.f8 ? (size_t)g.ld_k8 : g.ld_k * cs_of(p);  // bytes per forward-operand row
  char* sc = b.sbuf ? static_cast<char*>(b.sbuf) + (size_t)first * kTileElems * cs_of(p) : nullptr;
  launch_fwd_stats(comp, op_all + (size_t)p.rank * g.rows_pad * op_row, op_all, b.fwd_tiles + first, count, b.part, sc, ws, g, s,
                   BlockView{}, b.part_x, own ? std::min(count, own_diag_tail(g)) : 0);
}

void sym_lse(const SymPlan&, const Geometry& g, const SymBuffers& b, hipStream_t s) {
  NTXENT_TRACE("ntxent.lse");
  fault_point("lse");
  NTXENT_CHECK(b.part && b.ypos && b.lse2_all && b.cpos && b.block_loss && b.loss, "symmetric step: LSE buffer missing");
  launch_lse(b.part, b.ypos, b.lse2_all, b.cpos, b.block_loss, b.loss, g, s);
}

void sym_transpose_partners(const SymPlan& p, const Geometry& g, const SymBuffers& b, hipStream_t s) {
  NTXENT_TRACE("ntxent.transpose_partners");
  NTXENT_CHECK(b.zq_all && b.zqt_all, "symmetric step: transpose buffer missing");
  for (const SymJob& j : p.jobs)  // partners' B operands of the own dZ GEMMs
    launch_transpose(p.bwd, rows_of(p, g, b.zq_all, j.q), zqt_of(p, g, b.zqt_all, j.q), g, s);
}

void sym_coef(const SymPlan& p, const Geometry& g, const SymBuffers& b, hipStream_t s) {
  NTXENT_TRACE("ntxent.coef");
  fault_point("coef");
  NTXENT_CHECK(b.sbuf && b.cbuf && b.mbuf && b.lse2_all && b.cpos && b.fwd_tiles, "symmetric step: coefficient buffer missing");
  launch_coef(p.bwd, b.sbuf, b.cbuf, b.lse2_all, b.cpos, b.fwd_tiles, p.n_fwd, g, s, b.mbuf);
}

void sym_partner_grads(const SymPlan& p, const Geometry& g, const SymBuffers& b, const GemmWorkspace& ws, hipStream_t s) {
  NTXENT_TRACE("ntxent.dz_partners");
  fault_point("dz");
  for (const SymDzCall& c : p.partner_dz) dz_call(p, g, c, b, ws, s);
}

void sym_own_grads(const SymPlan& p, const Geometry& g, const SymBuffers& b, const GemmWorkspace& ws, hipStream_t s) {
  NTXENT_TRACE("ntxent.dz_own");
  for (const SymDzCall& c : p.own_dz) dz_call(p, g, c, b, ws, s);
}

void sym_norm_bwd(const SymPlan& p, const Geometry& g, DType in, const SymBuffers& b, hipStream_t s) {
  NTXENT_TRACE("ntxent.norm_bwd");
  fault_point("norm_bwd");
  const int ninc = (int)p.incoming.size();
  NTXENT_CHECK(b.own && b.h && b.inv && b.grad_out && b.dh && (!p.contrib_f16 || ninc == 0 || b.recv),
               "symmetric step: normalisation backward buffer missing");
  if (p.contrib_f16)
    launch_norm_bwd(in, b.own, 1, b.h, b.inv, b.grad_out, b.dh, g, s, b.recv, ninc);
  else
    launch_norm_bwd(in, b.own, 1 + ninc, b.h, b.inv, b.grad_out, b.dh, g, s);
}

}  // namespace ntxent
