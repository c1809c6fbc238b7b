"""Symmetric global-batch negatives: every rank pair's similarity block is computed ONCE.

The all-gather path (``parallel.distributed``) has every rank r compute its full row block
S_{r,:} = Z_r Z_all^T / tau, so each off-diagonal block S_{r,q} is computed twice in the group
(once as S_{r,q} by r, once as S_{q,r} = S_{r,q}^T by q). Here the W(W-1)/2 off-diagonal
blocks are split evenly: rank r computes the blocks (r, r+1), ..., (r, r+(W-1)//2) (mod W) in
full and, for even W, half of the block (r, r + W/2) (the pair shares it by row tiles). For
each tile of a block it computes, the forward GEMM epilogue emits the row partials (for r's
rows) AND the column partials (for q's rows), and the kept cosines give both coefficient
blocks C_{r,q} and C_{q,r} = C_{r,q}^T. This is the north star's "reduce-scatter of
embedding grads on the backward" (BASELINE.json), done point to point over xGMI:

* forward: prep -> Zq sent point-to-point to the ranks that compute against it (half of an
  all-gather's traffic: 4 x 32 MiB per rank at W = 8, one grouped batch so every peer's
  transfer runs on its own link at once) while the own upper-triangular tiles run -> the
  assigned cross tiles -> column partials (2 MiB per block at B=4096) sent to their owners ->
  LSE -> LSE all-gather + loss all-reduce.
* backward: partners' ZqT blocks transposed locally; coefficient pass (own tiles mirrored in
  place, cross tiles mirrored into a per-partner buffer) -> the partners' gradient contributions C_{q,r} Z_r (MFMA dZ GEMMs),
  sent point-to-point as soon as they exist (fp16 for reduced-precision plans: 32 MiB per
  block) -> this rank's own
  contributions C_{r,q} Z_q accumulate in the dZ epilogue while the sends run -> received
  contributions added -> L2-normalisation backward.

Per GPU at W = 8 (B = 4096/view, d = 2048) the forward similarity work drops from 7.5 to 4
blocks of 8192 x 8192 x 2048 and the coefficient pass from 7.5 to 4 blocks; the dZ GEMMs stay
at 8 blocks (half of them produce the partners' contributions). Traffic: 3.5 x 32 MiB of fp16
dZ contributions per rank, each to a different peer (one xGMI link each), overlapped with the
own-row dZ GEMMs.

The reference has no multi-GPU code at all; the math is SURVEY.md §2.2.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Tuple

import torch
import torch.distributed as dist

from ..ops import _ext, reference
from ..ops.ntxent import refuse_temperature_grad, resolve_compute
from .commstats import comm_reserve_cus, span
from .distributed import _all_gather_into, _is_gloo, _world

# The step itself (the block assignment, the schedule of chunks, exchanges and dZ calls, the buffer
# sizes and the launches) lives in csrc/runtime/sym_step.cpp, shared with the native Engine and
# the emulation. This module is the torch.distributed transport: it walks the plan's exchange
# lists and calls the phases between them.
Job = Tuple[int, int, int, int, int]  # (q, m0, m1, k0, k1): my row tiles [m0,m1) x q's row tiles [k0,k1)
TILE = 256


@functools.lru_cache(maxsize=None)
def _assignment(world: int, rank: int, row_tiles: int):
    p = _ext.load().sym_plan(row_tiles * TILE, 64, world, rank)  # the assignment depends on these three alone
    return tuple(p["jobs"]), tuple(p["incoming"])


def sym_jobs(world: int, rank: int, row_tiles: int) -> List[Job]:
    """Blocks rank ``rank`` computes: (q, m0, m1, k0, k1) = its row tiles [m0, m1) against
    rank q's row tiles [k0, k1). Every unordered pair {r, q} (r != q) is covered exactly once
    across the group (the rule is sym_jobs of sym_step.cpp)."""
    return list(_assignment(world, rank, row_tiles)[0])


def sym_incoming(world: int, rank: int, row_tiles: int) -> List[Job]:
    """Jobs of OTHER ranks that involve ``rank``'s rows: (p, m0, m1, k0, k1) with rank p
    computing its row tiles [m0, m1) against this rank's row tiles [k0, k1)."""
    return list(_assignment(world, rank, row_tiles)[1])


def sym_work_blocks(world: int, row_tiles: int) -> List[float]:
    """Cross-block tiles per rank in units of full blocks (balance check)."""
    return [sum((m1 - m0) * (k1 - k0) for (_, m0, m1, k0, k1) in sym_jobs(world, r, row_tiles)) / row_tiles ** 2
            for r in range(world)]


def _grank(group, r: int) -> int:
    return dist.get_global_rank(group, r) if group is not None else r


def _p2p(sends, recvs, group):
    """Point-to-point exchange: ``sends`` = [(tensor, dst)], ``recvs`` = [(tensor, src)] (group
    ranks). RCCL: one grouped batch on the communicator's stream, returns work handles. gloo
    (CPU transport for the 1-GPU rehearsals): host-staged isend/irecv, completed on return."""
    if not sends and not recvs:
        return []
    if _is_gloo(group):
        reqs, back = [], []
        for t, dst in sends:
            c = t.detach().contiguous().cpu()
            back.append(c)  # keep alive until sent
            reqs.append(dist.isend(c, _grank(group, dst), group=group))
        for t, src in recvs:
            c = torch.empty(t.shape, dtype=t.dtype)
            reqs.append(dist.irecv(c, _grank(group, src), group=group))
            back.append((t, c))
        for q in reqs:
            q.wait()
        for item in back:
            if isinstance(item, tuple):
                item[0].copy_(item[1])
        return []
    ops = [dist.P2POp(dist.isend, t, _grank(group, dst), group) for t, dst in sends]
    ops += [dist.P2POp(dist.irecv, t, _grank(group, src), group) for t, src in recvs]
    return dist.batch_isend_irecv(ops)


_STEPS: Dict[tuple, tuple] = {}


def sym_step(C, plan, device):
    """(SymStep, its schedule as a dict) of a shape, cached: the schedule is built and its tile
    lists are uploaded once. Exchange records are (send, peer, slot0, slot1, t0, t1, pack_off),
    see sym_step.h."""
    key = (plan.rows, plan.dim, plan.world, plan.rank, device.index, plan.compute_dtype)
    hit = _STEPS.get(key)
    if hit is None:
        S = C.sym_step(plan)
        hit = _STEPS[key] = (S, S.plan)
    return hit


def contrib_dtype(plan) -> torch.dtype:
    """dtype of the partner gradient contributions on the wire: fp16 for the reduced-precision
    plans (half the xGMI bytes; the contributions are O(1) sums, fp16's 11-bit mantissa is
    finer than the bf16/fp16 gradient they end up in), fp32 for exact-fp32 plans."""
    return torch.float32 if plan.backward_dtype == "fp32" else torch.float16


def _cdt(plan) -> torch.dtype:
    return {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[plan.backward_dtype]


def _buf(sp, name: str, dtype: torch.dtype, device) -> torch.Tensor:
    return torch.empty((sp["bytes"][name] // dtype.itemsize,), dtype=dtype, device=device)


def sym_forward_bufs(sp, plan, h: torch.Tensor, zq_all, zqt_all, zq8_all=None) -> dict:
    """The forward's bundle over the (shared or gathered) row buffers."""
    dev, Rpad = h.device, plan.rows_pad
    f32 = dict(dtype=torch.float32, device=dev)
    B = {"h": h, "zq_all": zq_all, "zqt_all": zqt_all, "inv": torch.empty((plan.rows,), **f32),
         "ypos": torch.empty((plan.rows,), **f32), "part": torch.empty((plan.col_tiles, Rpad, 2), **f32),
         "part_x": torch.empty((plan.col_tiles, Rpad, 2), **f32), "sbuf": _buf(sp, "sbuf", _cdt(plan), dev)}
    if zq8_all is not None:
        B["zq8_all"] = zq8_all
    return B


def sym_lse(S, plan, B, lse2_all) -> torch.Tensor:
    """LSE of this rank's rows into its slot of ``lse2_all``; B gains cpos and the local loss."""
    B.update(lse2_all=lse2_all, cpos=torch.empty((plan.rows_pad,), dtype=torch.float32, device=lse2_all.device),
             loss=torch.empty((), dtype=torch.float32, device=lse2_all.device))
    S.lse(plan, B)
    return B["loss"]


def sym_partner_contribs(S, sp, plan, B) -> torch.Tensor:
    """Coefficient pass (B: sbuf, lse2_all, cpos) and the partners' contributions C_{q,r} Z_r: one
    slab per job, [jobs, Rpad, dim_n] in :func:`contrib_dtype`. The kept cosines are released
    before the dZ GEMMs; B keeps cbuf for :meth:`own_grads`."""
    dev = B["lse2_all"].device
    B.update(cbuf=_buf(sp, "cbuf", _cdt(plan), dev), mbuf=_buf(sp, "mbuf", _cdt(plan), dev))
    S.coef(plan, B)
    del B["sbuf"]
    B["contrib"] = torch.empty((len(sp["jobs"]), plan.rows_pad, plan.dim_n), dtype=contrib_dtype(plan), device=dev)
    S.partner_grads(plan, B)
    return B["contrib"]


def sym_grad_slabs(sp, plan, device):
    """(own, received): own = fp32 [1, Rpad, dim_n] for this rank's contributions; received =
    [incoming, Rpad, dim_n] in :func:`contrib_dtype`, slab i = what incoming job i sends, rows
    outside its range zeroed (the memory is fresh every step). The normalisation backward sums
    them all while reading."""
    own = torch.empty((1, plan.rows_pad, plan.dim_n), dtype=torch.float32, device=device)
    recv = torch.empty((len(sp["incoming"]), plan.rows_pad, plan.dim_n), dtype=contrib_dtype(plan), device=device)
    for (send, _, i, _, t0, t1, _) in sp["contribs"]:
        if not send:
            recv[i, :t0 * TILE].zero_()
            recv[i, t1 * TILE:].zero_()
    return own, recv


def sym_contrib_views(sp, contrib, recv):
    """The contribution exchange as ([(rows to send, peer)], [(rows to receive into, peer)]); a
    side given as None is left out."""
    sends = [(contrib[i, t0 * TILE:t1 * TILE], q) for (send, q, i, _, t0, t1, _) in sp["contribs"]
             if send and contrib is not None]
    recvs = [(recv[i, t0 * TILE:t1 * TILE], p) for (send, p, i, _, t0, t1, _) in sp["contribs"]
             if not send and recv is not None]
    return sends, recvs


def sym_norm_bwd(S, plan, own, recv, h, inv, grad_out) -> torch.Tensor:
    dh = torch.empty_like(h)
    B = {"h": h, "dh": dh, "inv": inv, "grad_out": grad_out.reshape(1).to(torch.float32).contiguous()}
    if recv.dtype == torch.float32:  # exact-fp32 plans: one fp32 stack
        B["own"] = torch.cat([own, recv], 0)
    else:
        B.update(own=own, recv=recv)
    S.norm_bwd(plan, B)
    return dh


class SymNTXentFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h: torch.Tensor, temperature: float, compute: str, group):
        C = _ext.load()
        W, r = _world(group)
        h = h.contiguous()
        R, d = h.shape
        plan = C.get_plan(R, d, W, r, float(temperature), compute, h.device.index)
        dev, Rpad = h.device, plan.rows_pad
        S, sp = sym_step(C, plan, dev)
        f8 = plan.compute_dtype == "fp8"
        zq_all = torch.empty((W * Rpad, plan.ld_k), dtype=_cdt(plan), device=dev)
        zqt_all = torch.empty((W, plan.dim_n, plan.ld_t), dtype=_cdt(plan), device=dev)
        fwd_all = torch.empty((W * Rpad, plan.ld_k8), dtype=torch.uint8, device=dev) if f8 else zq_all
        B = sym_forward_bufs(sp, plan, h, zq_all, zqt_all, fwd_all if f8 else None)
        S.prep(plan, B)
        # rows travel only where a block needs them: to the ranks that compute against this
        # rank's rows (only the row tiles they use) and from the ranks this one computes
        # against -- half of an all-gather's traffic. Chunk c of the rows is one grouped batch
        # (RCCL runs a group's peers concurrently over their own xGMI links; the chunks follow
        # each other on the communicator's stream), and the cross tiles of chunk c run while
        # chunk c+1 is on the wire. The partners' ZqT blocks are transposed locally in the
        # backward.

        def rows(xs, buf):  # row tiles [t0, t1) of the sender's slot
            return ([(buf[r * Rpad + t0 * TILE:r * Rpad + t1 * TILE], p) for (send, p, _, _, t0, t1, _) in xs if send],
                    [(buf[q * Rpad + t0 * TILE:q * Rpad + t1 * TILE], q) for (send, q, _, _, t0, t1, _) in xs if not send])

        works = [_p2p(*rows(xs, fwd_all), group) for xs in sp["rows"]]
        works_f16 = _p2p(*rows(sp["rows_f16"], zq_all), group)  # fp8: the backward runs on the fp16 rows
        reserve = comm_reserve_cus(dist.get_backend(group))
        # chunk 0 of the rows is on the wire
        S.fwd_tiles_range(plan, B, 0, sp["n_own"], reserve_cus=reserve)
        for c, (ws, (first, count)) in enumerate(zip(works, sp["segs"])):
            with span("fwd_rows"):
                for w in ws:
                    w.wait()
            # the next chunk (or the fp16 rows of an fp8 plan) is still on the wire
            more = c + 1 < len(works) and bool(works[c + 1]) or bool(works_f16)
            S.fwd_tiles_range(plan, B, first, count, reserve_cus=reserve if more else 0)
        with span("fwd_rows"):
            for w in works_f16:
                w.wait()
        # column partials of the cross tiles -> their rows' owners
        part, part_x = B["part"], B["part_x"]
        sends = [(part_x[s0:s1, t0 * TILE:t1 * TILE].contiguous(), q)
                 for (send, q, s0, s1, t0, t1, _) in sp["col_partials"] if send]
        into = [(part[s0:s1, t0 * TILE:t1 * TILE], p) for (send, p, s0, s1, t0, t1, _) in sp["col_partials"] if not send]
        recvs = [(torch.empty(v.shape, dtype=torch.float32, device=dev), p) for v, p in into]
        with span("fwd_col_partials"):
            for w in _p2p(sends, recvs, group):
                w.wait()
        for (buf, _), (v, _) in zip(recvs, into):
            v.copy_(buf)
        lse2_all = torch.empty((W * Rpad,), dtype=torch.float32, device=dev)
        loss = sym_lse(S, plan, B, lse2_all)
        mine = lse2_all[r * Rpad:(r + 1) * Rpad].clone()
        with span("lse_loss"):
            _all_gather_into(lse2_all, mine, group)
            dist.all_reduce(loss, op=dist.ReduceOp.SUM, group=group)
        ctx.plan, ctx.group = plan, group
        ctx.sc = B["sbuf"]
        ctx.save_for_backward(h, B["inv"], zq_all, zqt_all, lse2_all, B["cpos"])
        return loss

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        """The partners' contributions first (one stacked GEMM), sent in one grouped batch
        (concurrent over the peers' links) while this rank's own dZ GEMMs run; received
        contributions land in their own slabs, summed by the normalisation backward."""
        C = _ext.load()
        h, inv, zq_all, zqt_all, lse2_all, cpos = ctx.saved_tensors
        plan, group = ctx.plan, ctx.group
        B = {"zq_all": zq_all, "zqt_all": zqt_all, "lse2_all": lse2_all, "cpos": cpos, "sbuf": ctx.sc}
        ctx.sc = None
        if B["sbuf"] is None:
            raise RuntimeError("symmetric NT-Xent: backward called twice (kept cosines already consumed)")
        S, sp = sym_step(C, plan, h.device)
        S.transpose_partners(plan, B)  # partners' B operands of the own dZ GEMMs
        contrib = sym_partner_contribs(S, sp, plan, B)
        B["own"], recv = sym_grad_slabs(sp, plan, h.device)
        works = _p2p(*sym_contrib_views(sp, contrib, recv), group)
        S.own_grads(plan, B, reserve_cus=comm_reserve_cus(dist.get_backend(group)) if works else 0)
        with span("bwd_partner_grads"):
            for w in works:
                w.wait()
        own = B["own"]
        del contrib, B  # the coefficient, mirror and contribution buffers go before the last launch
        return sym_norm_bwd(S, plan, own, recv, h, inv, grad_out), None, None, None


def sym_ntxent_loss(h_local: torch.Tensor, temperature: float = 0.07, *, group=None, compute: str = "auto",
                    use_mixed_precision: bool = False) -> torch.Tensor:
    """Global NT-Xent over the group with each rank pair's similarity block computed once;
    same value and gradient as :func:`parallel.distributed.dist_ntxent_loss`."""
    refuse_temperature_grad(temperature, "sym_ntxent_loss")
    W, _ = _world(group)
    if not h_local.is_cuda:
        return cpu_sym_ntxent_loss(h_local, temperature, group=group)
    comp = resolve_compute(h_local.dtype, use_mixed_precision, compute)
    if W == 1:
        from ..ops.ntxent import ntxent_loss

        return ntxent_loss(h_local, temperature, compute=comp)
    return SymNTXentFunction.apply(h_local, float(temperature), comp, group)


# ---------------------------------------------------------------------------------------
# CPU / gloo path: the same block assignment and exchanges with torch ops, at a configurable
# tile size (tests use small tiles so that the split pair and partial ranges are exercised).
# ---------------------------------------------------------------------------------------
class _CpuSymFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, temperature, group, tile):
        W, r = _world(group)
        R = h.shape[0]
        n = R // 2
        rt = -(-R // tile)
        Rp = rt * tile
        z, inv = reference.normalize(h)
        zp = torch.zeros((Rp, z.shape[1]), dtype=z.dtype)
        zp[:R] = z
        if W > 1:
            parts = [torch.empty_like(zp) for _ in range(W)]
            dist.all_gather(parts, zp, group=group)
        else:
            parts = [zp]
        valid = torch.arange(Rp) < R
        ninf = float("-inf")
        S_own = zp @ zp.t() / temperature
        S_own[~valid] = ninf
        S_own[:, ~valid] = ninf
        S_own.fill_diagonal_(ninf)
        lse_terms = [torch.logsumexp(S_own, 1)]
        jobs = sym_jobs(W, r, rt)
        inc = sym_incoming(W, r, rt)
        blocks = []
        col_sends = []
        for (q, m0, m1, k0, k1) in jobs:
            rows = slice(m0 * tile, m1 * tile)
            cols = slice(k0 * tile, k1 * tile)
            S = zp[rows] @ parts[q][cols].t() / temperature
            S[~valid[rows]] = ninf
            S[:, ~valid[cols]] = ninf
            blocks.append(S)
            t = torch.full((Rp,), ninf, dtype=S.dtype)
            t[rows] = torch.logsumexp(S, 1)
            lse_terms.append(t)
            col_sends.append((torch.logsumexp(S, 0), q))
        col_recvs = [(torch.empty(((k1 - k0) * tile,), dtype=z.dtype), p) for (p, m0, m1, k0, k1) in inc]
        _p2p(col_sends, col_recvs, group)
        for (buf, _), (p, m0, m1, k0, k1) in zip(col_recvs, inc):
            t = torch.full((Rp,), ninf, dtype=z.dtype)
            t[k0 * tile:k1 * tile] = buf
            lse_terms.append(t)
        lse = torch.logsumexp(torch.stack(lse_terms), 0)[:R]
        ar = torch.arange(R)
        pos = (ar + n) % R
        ypos = (z[ar] * z[pos]).sum(1) / temperature
        loss = (lse - ypos).sum() / (W * R)
        if W > 1:
            lparts = [torch.empty_like(lse) for _ in range(W)]
            dist.all_gather(lparts, lse.contiguous(), group=group)
            dist.all_reduce(loss, group=group)
        else:
            lparts = [lse]
        ctx.save_for_backward(z, inv)
        ctx.meta = (temperature, W, r, tile, group, parts, blocks, lparts, S_own)
        return loss

    @staticmethod
    def backward(ctx, g):
        z, inv = ctx.saved_tensors
        temperature, W, r, tile, group, parts, blocks, lparts, S_own = ctx.meta
        R = z.shape[0]
        n = R // 2
        rt = -(-R // tile)
        Rp = rt * tile

        def padl(l):
            out = torch.full((Rp,), float("inf"), dtype=l.dtype)  # exp(S - inf) = 0 on padding
            out[:R] = l
            return out

        lse_all = [padl(l) for l in lparts]
        lr = lse_all[r]
        Cown = torch.exp(S_own - lr[:, None]) + torch.exp(S_own - lr[None, :])
        ar = torch.arange(R)
        Cown[ar, (ar + n) % R] -= 2.0
        dz = Cown @ parts[r]
        jobs = sym_jobs(W, r, rt)
        inc = sym_incoming(W, r, rt)
        sends = []
        for (q, m0, m1, k0, k1), S in zip(jobs, blocks):
            rows = slice(m0 * tile, m1 * tile)
            cols = slice(k0 * tile, k1 * tile)
            Cb = torch.exp(S - lr[rows, None]) + torch.exp(S - lse_all[q][None, cols])
            dz[rows] += Cb @ parts[q][cols]
            sends.append((Cb.t() @ parts[r][rows], q))
        recvs = [(torch.empty(((k1 - k0) * tile, z.shape[1]), dtype=z.dtype), p) for (p, m0, m1, k0, k1) in inc]
        _p2p(sends, recvs, group)
        for (buf, _), (p, m0, m1, k0, k1) in zip(recvs, inc):
            dz[k0 * tile:k1 * tile] += buf
        dz = dz[:R] * (g / (W * R * temperature))
        dot = (z * dz).sum(1, keepdim=True)
        return inv.unsqueeze(1) * (dz - z * dot), None, None, None


def cpu_sym_ntxent_loss(h_local: torch.Tensor, temperature: float = 0.07, group=None, tile: int = 256) -> torch.Tensor:
    refuse_temperature_grad(temperature, "cpu_sym_ntxent_loss")
    return _CpuSymFn.apply(h_local, float(temperature), group, int(tile))
