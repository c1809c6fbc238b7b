"""Symmetric data-parallel mode (parallel/symmetric.py) on CPU: the block assignment covers
every rank pair's similarity block exactly once and balances the work; W gloo processes
running the torch implementation of the same exchanges (column partials forward, partner
gradient contributions backward) reproduce the single-process fp64 oracle."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ntxent_amd.parallel.symmetric import sym_incoming, sym_jobs, sym_work_blocks


@pytest.mark.parametrize("W", range(1, 10))
@pytest.mark.parametrize("rt", [1, 2, 3, 4, 7, 32])
def test_assignment_covers_each_pair_once(W, rt):
    cover = {}
    for r in range(W):
        for (q, m0, m1, k0, k1) in sym_jobs(W, r, rt):
            assert q != r and 0 <= q < W
            assert 0 <= m0 < m1 <= rt and 0 <= k0 < k1 <= rt
            for i in range(m0, m1):
                for j in range(k0, k1):
                    key = (min(r, q), max(r, q), i if r < q else j, j if r < q else i)
                    assert key not in cover, f"block tile {key} computed twice"
                    cover[key] = r
    assert len(cover) == W * (W - 1) // 2 * rt * rt
    work = sym_work_blocks(W, rt)
    if W > 1:
        assert max(work) - min(work) <= 1.0 / rt + 1e-9  # at most one row-tile panel apart
        assert abs(sum(work) - W * (W - 1) / 2) < 1e-9


@pytest.mark.parametrize("W", range(2, 9))
def test_incoming_mirrors_jobs(W):
    rt = 5
    for r in range(W):
        for (p, m0, m1, k0, k1) in sym_incoming(W, r, rt):
            assert (r, m0, m1, k0, k1) in sym_jobs(W, p, rt)
    n_msgs = sum(len(sym_jobs(W, r, rt)) for r in range(W))
    assert n_msgs == sum(len(sym_incoming(W, r, rt)) for r in range(W))


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n, dim, T, grad_out, tile, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ntxent_amd.parallel.symmetric import cpu_sym_ntxent_loss

        g = torch.Generator().manual_seed(2000 + rank)
        h = torch.randn(2 * n, dim, generator=g, dtype=torch.float64).requires_grad_(True)
        loss = cpu_sym_ntxent_loss(h, T, tile=tile)
        loss.backward(torch.tensor(grad_out, dtype=torch.float64))
        q.put((rank, loss.detach().numpy().copy(), h.detach().numpy().copy(), h.grad.detach().numpy().copy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,dim,tile", [(2, 4, 8, 2), (2, 5, 7, 3), (3, 3, 6, 2), (4, 3, 5, 2), (4, 4, 6, 8)])
def test_gloo_symmetric_matches_oracle(world, n, dim, tile):
    from ntxent_amd.ops import reference as ref

    T, go = 0.1, 0.7
    ctx = mp.get_context("spawn")
    qu = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, dim, T, go, tile, qu)) for r in range(world)]
    for p in procs:
        p.start()
    out = [qu.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    res = [(r, torch.from_numpy(l), torch.from_numpy(h), torch.from_numpy(g)) for r, l, h, g in sorted(out, key=lambda x: x[0])]
    shards = [r[2] for r in res]
    hg = ref.global_pair_order(shards).requires_grad_(True)
    l_ref = ref.ntxent_loss(hg, T)
    (g_ref,) = torch.autograd.grad(l_ref, hg, torch.tensor(go, dtype=hg.dtype))
    N = world * n
    for r, (_, loss, _, grad) in enumerate(res):
        torch.testing.assert_close(loss, l_ref.detach(), rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(grad[:n], g_ref[r * n:(r + 1) * n], rtol=1e-9, atol=1e-12)
        torch.testing.assert_close(grad[n:], g_ref[N + r * n:N + (r + 1) * n], rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------------------------------
# The schedule of the symmetric step (csrc/runtime/sym_step.cpp) through the plan binding: what
# the Engine, the autograd path and the emulation all walk.
# ---------------------------------------------------------------------------------------
SHAPES = [(W, rt) for W in range(1, 10) for rt in (1, 2, 3, 4, 7, 32)]
DIM = 64
TILE_BYTES = 256 * 256 * 2  # fp16 plans


def _plan(W, r, rt, compute="fp16"):
    from ntxent_amd.ops import _ext

    return _ext.load().sym_plan(rt * 256, DIM, W, r, compute)


def _frozen_sym_jobs(world, rank, row_tiles):
    """The assignment rule, frozen: the specification sym_step.cpp's sym_jobs is held to."""
    W, r, rt = world, rank, row_tiles
    jobs = []
    for d in range(1, (W - 1) // 2 + 1):
        jobs.append(((r + d) % W, 0, rt, 0, rt))
    if W % 2 == 0 and W > 1:
        q = (r + W // 2) % W
        h = (rt + 1) // 2
        job = (q, 0, h, 0, rt) if r < q else (q, 0, rt, h, rt)
        if job[1] < job[2] and job[3] < job[4]:
            jobs.append(job)
    return jobs


@pytest.mark.parametrize("W,rt", SHAPES)
def test_plan_assignment_is_pinned(W, rt):
    for r in range(W):
        p = _plan(W, r, rt)
        assert p["jobs"] == _frozen_sym_jobs(W, r, rt) == sym_jobs(W, r, rt)
        inc = [(q, m0, m1, k0, k1) for q in range(W) if q != r
               for (t, m0, m1, k0, k1) in _frozen_sym_jobs(W, q, rt) if t == r]
        assert p["incoming"] == inc == sym_incoming(W, r, rt)
        assert p["nchunks"] == max(1, min(4, rt))


@pytest.mark.parametrize("W,rt", SHAPES)
def test_plan_chunk_segments(W, rt):
    from ntxent_amd.ops import _ext

    for r in range(W):
        p = _plan(W, r, rt)
        tiles = _ext.load().sym_fwd_tile_list(rt * 256, DIM, W, r)
        nch, at = p["nchunks"], p["n_own"]
        assert p["n_own"] == rt * (rt + 1) // 2 and len(p["segs"]) == nch and p["n_fwd"] == len(tiles)
        for c, (first, count) in enumerate(p["segs"]):
            assert first == at and count >= 0
            at += count
            for (ti, tj, kind) in tiles[first:first + count]:
                assert rt * c // nch <= tj % rt < rt * (c + 1) // nch and tj // rt != r
        assert at == len(tiles)


def _messages(p, key, chunk=None):
    xs = p[key] if chunk is None else p[key][chunk]
    assert [x[0] for x in xs] == sorted((x[0] for x in xs), reverse=True), "sends come first"
    return xs


@pytest.mark.parametrize("compute", ["fp16", "fp32", "fp8"])
@pytest.mark.parametrize("W,rt", SHAPES)
def test_plan_exchanges_match_across_ranks(W, rt, compute):
    from ntxent_amd.ops import _ext

    g = _ext.load().geometry(rt * 256, DIM, W, 0)
    Rpad, f2 = g["rows_pad"], 8
    plans = [_plan(W, r, rt, compute) for r in range(W)]
    lists = [("rows", c) for c in range(plans[0]["nchunks"])] + [("rows_f16", None), ("col_partials", None), ("contribs", None)]
    for key, chunk in lists:
        for r in range(W):
            p, nb = plans[r], plans[r]["bytes"]
            xs = _messages(p, key, chunk)
            assert (key != "rows_f16") or (bool(xs) == (compute == "fp8" and W > 1))
            for (send, q, s0, s1, t0, t1, off) in xs:
                assert q != r and 0 <= q < W and 0 <= t0 < t1 <= rt
                if key == "col_partials":
                    base = q * rt  # send: the partner's slots of part_x; receive: the sender's slots of part
                    assert base <= s0 < s1 <= base + rt and s1 * Rpad * f2 <= nb["part_x"]
                    if off >= 0:
                        assert t1 - t0 < rt and (off + (s1 - s0) * (t1 - t0) * 256) * f2 <= nb["xsend" if send else "xrecv"]
                    else:
                        assert (t0, t1) == (0, rt)
                elif key == "contribs":
                    row = nb["slab"] // Rpad
                    if send:
                        assert s0 * nb["slab"] + t1 * 256 * row <= nb["contrib"]
                    elif p["contrib_f16"]:
                        assert s0 * nb["slab"] + t1 * 256 * row <= nb["recv"]
                    else:
                        assert nb["recv"] == 0 and (1 + s0) * nb["slab"] + t1 * 256 * row <= nb["own"]
            for q in range(W):
                out = [(s1 - s0, t0, t1) for (send, peer, s0, s1, t0, t1, _) in xs if send and peer == q]
                back = [(s1 - s0, t0, t1) for (send, peer, s0, s1, t0, t1, _) in _messages(plans[q], key, chunk)
                        if not send and peer == r]
                assert out == back, (key, chunk, r, q)  # count, order and size (same rows, same row bytes)
                if key == "col_partials":  # the same row tiles m of the sender on both sides
                    a = [s0 - q * rt for (send, peer, s0, *_) in xs if send and peer == q]
                    b = [s0 - r * rt for (send, peer, s0, *_) in plans[q][key] if not send and peer == r]
                    assert a == b
    # every job's rows travel exactly once over the chunks
    for r in range(W):
        got = sorted((q, t) for c in range(plans[r]["nchunks"]) for (send, q, _, _, t0, t1, _) in plans[r]["rows"][c]
                     if not send for t in range(t0, t1))
        assert got == sorted((q, t) for (q, m0, m1, k0, k1) in plans[r]["jobs"] for t in range(k0, k1))


def _b_tile(call, kt, rt):
    """Global row tile of Z the K tile kt of a dZ call reads."""
    (_, _, _, b_block0, b_col0, kblk, k_tiles, *_rest) = call
    assert b_col0 % 256 == 0 and kblk % 256 == 0 and kblk <= rt * 256
    col = kt * 256
    if k_tiles * 256 > kblk:  # whole consecutive blocks
        assert b_col0 == 0 and kblk == rt * 256
    blk, within = b_block0 + col // kblk, b_col0 + col % kblk
    assert within < rt * 256
    return blk * rt + within // 256


@pytest.mark.parametrize("W,rt", SHAPES)
def test_plan_dz_calls_cover_the_coefficients_once(W, rt):
    from ntxent_amd.ops import _ext

    for r in range(W):
        p, nb = _plan(W, r, rt), _plan(W, r, rt)["bytes"]
        col_tiles, c_ld, jobs = W * rt, p["c_ld"], p["jobs"]
        dim_n = _ext.load().geometry(rt * 256, DIM, W, r)["dim_n"]
        tn = dim_n // 256
        assert nb["dz_rows"] == len(p["dz_rows"]) * 16
        # own calls: every coefficient tile this rank holds feeds its output row tile once
        want = {(m, r * rt + k) for m in range(rt) for k in range(rt)}
        want |= {(m, q * rt + k) for (q, m0, m1, k0, k1) in jobs for m in range(m0, m1) for k in range(k0, k1)}
        seen, touched = set(), set()
        for call in p["own_dz"]:
            (mirror, a0, panel, b_block0, b_col0, kblk, k_tiles, m0, m1, out, accum, off) = call
            assert not mirror and out == -1 and panel == c_ld and 0 <= m0 < m1 <= rt and k_tiles > 0
            assert p["dz_rows"][off:off + (m1 - m0) * tn] == [(m, n) for m in range(m0, m1) for n in range(tn)]
            for m in range(m0, m1):
                assert accum == (m in touched), "first call into a row tile overwrites, later ones accumulate"
                for kt in range(k_tiles):
                    a = a0 + m * panel + kt
                    assert a // c_ld == m and (a + 1) * TILE_BYTES <= nb["cbuf"]
                    nt = (a % c_ld + r * rt) % col_tiles  # compact layout: slot (nt - rank * rt) mod col_tiles
                    assert _b_tile(call, kt, rt) == nt and nt < col_tiles
                    assert (m, nt) not in seen
                    seen.add((m, nt))
            touched |= set(range(m0, m1))
        assert seen == want and touched == set(range(rt))
        assert nb["own"] == rt * 256 * dim_n * 4 and nb["slab"] == rt * 256 * dim_n * 2  # fp32 own slab, fp16 on the wire
        # partner calls: every (k of q, m of r) of each job feeds row tile k of q's slab once
        want = {(i, k, m) for i, (q, m0, m1, k0, k1) in enumerate(jobs) for m in range(m0, m1) for k in range(k0, k1)}
        seen = set()
        for call in p["partner_dz"]:
            (mirror, a0, panel, b_block0, b_col0, kblk, k_tiles, m0, m1, out, accum, off) = call
            assert mirror and out >= 0 and not accum and panel == rt and 0 <= m0 < m1 and k_tiles > 0
            assert p["dz_rows"][off:off + (m1 - m0) * tn] == [(m, n) for m in range(m0, m1) for n in range(tn)]
            for mt in range(m0, m1):
                slab, k_out = out + mt // rt, mt % rt
                assert (slab + 1) * nb["slab"] <= nb["contrib"]
                for kt in range(k_tiles):
                    a = a0 + mt * panel + kt
                    assert (a + 1) * TILE_BYTES <= nb["mbuf"]
                    slot, k, m = a // (rt * rt), a % (rt * rt) // rt, a % rt  # mirror slot (q - rank - 1) mod W
                    q = (slot + r + 1) % W
                    assert jobs[slab][0] == q and k == k_out
                    assert _b_tile(call, kt, rt) == r * rt + m
                    assert (slab, k, m) not in seen
                    seen.add((slab, k, m))
        assert seen == want
        assert p["split"] == (len(jobs) > p["nfull"]) and len(p["partner_dz"]) == (p["nfull"] > 0) + p["split"]
