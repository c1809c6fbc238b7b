"""Host-side planning logic of the HIP path (runs on CPU: no device needed).

Checks the invariants the kernels rely on: the forward tile list covers every (row, column)
tile pair exactly once counting the mirrored lower triangle of the own-rank block, the dZ
tiles cover the output, and the persistent stream-K schedule covers every K-step of every
tile exactly once with the per-block work balanced.
"""
import pytest

from ntxent_amd.ops import _ext


@pytest.fixture(scope="module")
def C():
    return _ext.load()


@pytest.mark.parametrize("rows,dim", [(64, 128), (34, 100), (8192, 2048), (600, 200), (2048, 8192)])
def test_geometry(C, rows, dim):
    g = C.geometry(rows, dim)
    assert g["rows_pad"] % C.TILE == 0 and g["rows_pad"] >= rows > g["rows_pad"] - C.TILE
    assert g["dim_k"] % 64 == 0 and g["dim_k"] >= dim
    assert g["dim_n"] % C.TILE == 0 and g["dim_n"] >= g["dim_k"]
    assert g["ld_k"] >= g["dim_k"] and g["ld_t"] >= g["rows_pad"]
    # de-aliased strides: never a multiple of 1024 elements
    assert g["ld_k"] % 1024 != 0 and g["ld_t"] % 1024 != 0
    assert g["col_tiles"] == g["row_tiles"] and g["global_rows"] == rows


def test_geometry_rejects_bad_input(C):
    with pytest.raises(Exception):
        C.geometry(7, 16)
    with pytest.raises(Exception):
        C.geometry(8, 16, 2, 2)
    with pytest.raises(Exception):
        C.geometry(8, 0)


@pytest.mark.parametrize("rows,world,rank", [(512, 1, 0), (8192, 1, 0), (1024, 4, 2), (300, 2, 1), (8192, 8, 7)])
def test_fwd_tiles_cover_once(C, rows, world, rank):
    g = C.geometry(rows, 64, world, rank)
    tiles = C.fwd_tile_list(rows, 64, world, rank)
    own = rank * g["row_tiles"]
    covered = {}
    for ti, tj, kind in tiles:
        local = tj - own
        if 0 <= local < g["row_tiles"]:
            assert local >= ti
            assert kind == (1 if local == ti else 2)
            covered[(ti, tj)] = covered.get((ti, tj), 0) + 1
            if local != ti:
                covered[(local, own + ti)] = covered.get((local, own + ti), 0) + 1
        else:
            assert kind == 0
            covered[(ti, tj)] = covered.get((ti, tj), 0) + 1
    assert len(covered) == g["row_tiles"] * g["col_tiles"]
    assert set(covered.values()) == {1}
    rt = g["row_tiles"]
    assert len(tiles) == rt * (g["col_tiles"] - rt) + rt * (rt + 1) // 2
    # the own block ends with its diagonal tiles (the strip kernel's remainder, launch_fwd_stats)
    n_own = rt * (rt + 1) // 2
    assert [t[2] for t in tiles[n_own - rt:n_own]] == [1] * rt
    assert [t[0] for t in tiles[n_own - rt:n_own]] == list(range(rt))


def test_dz_tiles_cover_output(C):
    g = C.geometry(1024, 600)
    tiles = C.dz_tile_list(1024, 600)
    assert sorted((t[0], t[1]) for t in tiles) == [(i, j) for i in range(g["row_tiles"]) for j in range(g["dim_n"] // C.TILE)]


@pytest.mark.parametrize("ntiles,nk,cus", [(528, 32, 256), (256, 128, 256), (10, 4, 256), (1, 3, 256),
                                           (300, 7, 256), (136, 16, 80), (1000, 2, 256), (36, 128, 256),
                                           (528, 8, 256), (2080, 16, 256)])
def test_stream_k_schedule(C, ntiles, nk, cus):
    s = C.schedule(ntiles, nk, cus)
    G = s["grid"]
    assert 1 <= G <= cus
    assert s["dp_tiles"] + s["sk_tiles"] == ntiles
    assert s["dp_tiles"] % G == 0  # whole data-parallel rounds
    # only the remainder of the DP rounds is split
    assert s["sk_tiles"] == ntiles % cus
    # every stream-K iteration is owned by exactly one block, contiguous ranges
    total = s["sk_tiles"] * nk
    if total:
        ipb = s["ipb"]
        assert G * ipb >= total
        owned = 0
        pieces = {}
        for b in range(G):
            lo, hi = b * ipb, min((b + 1) * ipb, total)
            owned += max(0, hi - lo)
            for t in range(lo // nk, (hi - 1) // nk + 1) if hi > lo else []:
                pieces[t] = pieces.get(t, 0) + 1
        assert owned == total
        # few contributors per split tile: the split p minimises nk/p + (p > 1: 10 + 4 (p - 1))
        # (make_schedule's cost model); the last arriver sums at most p + 1 slabs
        cands = range(1, max(1, min(cus // s["sk_tiles"], nk)) + 1)
        p_opt = min(cands, key=lambda c: (nk / c + (10 + 4 * (c - 1) if c > 1 else 0), c))
        assert max(pieces.values()) <= p_opt + 1
        assert s["ipb"] == -(-nk // p_opt)
    # balance: the busiest block does at most one DP round + ipb steps more than the mean
    mean = ntiles * nk / G
    worst = (s["dp_tiles"] // G) * nk + s["ipb"]
    assert worst <= mean + nk + 1


def test_workspace_bytes(C):
    # fixed layout: 2*num_cus arrival counters (stream-K splits < 2G tiles) + 2 fp32 tiles per block,
    # independent of the launch's tile count so launches can share one zero-initialised workspace
    b = C.gemm_workspace_bytes(528, 256)
    assert b >= 2 * 256 * 4 + 2 * 256 * 256 * 256 * 4
    assert b == C.gemm_workspace_bytes(7696, 256) == C.gemm_workspace_bytes(1, 256)
    for nt, nk in [(528, 32), (7696, 32), (300, 7), (255, 3)]:
        assert C.schedule(nt, nk, 256)["sk_tiles"] <= 2 * 256


def _panels_per_group(tiles, n_own, group=32):
    """Mean distinct Zq row panels (A and B) over consecutive `group`-tile runs of the own block:
    the L2 footprint of one XCD's share of a GEMM round (XCD-contiguous block mapping)."""
    own = [t for t in tiles[:n_own]]
    counts = []
    for s in range(0, len(own) - group + 1, group):
        counts.append(len({t[0] for t in own[s:s + group]} | {t[1] for t in own[s:s + group]}))
    return sum(counts) / len(counts)


def _zorder_list(rt):
    """The Z-order (Morton) own-block list the superblock order replaced (kept here as the
    reference: the off-diagonal upper tiles by Morton key, then the diagonal tail)."""
    def key(i, j):
        r = 0
        for b in range(16):
            r |= ((i >> b) & 1) << (2 * b + 1) | ((j >> b) & 1) << (2 * b)
        return r
    off = sorted([(i, j, 2) for i in range(rt) for j in range(i + 1, rt)], key=lambda t: key(t[0], t[1]))
    return off + [(i, i, 1) for i in range(rt)]


@pytest.mark.parametrize("rows", [8192, 16384, 2048, 6144])
def test_superblock_order_covers_same_tiles_with_fewer_panels(C, rows):
    """own_block_tiles: 8-panel superblocks (row-tile counts that are multiples of 8, >= 16; else
    the Z-order fallback) list the same tiles as Z-order with the diagonal tail last, and touch
    fewer distinct panels per 32-tile group (13.2 vs 15.4 at 32 row tiles)."""
    g = C.geometry(rows, 64, 1, 0)
    rt = g["row_tiles"]
    n_own = rt * (rt + 1) // 2
    a = [tuple(t) for t in C.fwd_tile_list(rows, 64, 1, 0)]
    b = _zorder_list(rt)
    assert sorted(a) == sorted(b) and len(set(a)) == len(a)
    assert a[n_own - rt:n_own] == b[n_own - rt:n_own] == [(i, i, 1) for i in range(rt)]
    if rt % 8 == 0 and rt >= 16:
        assert a != b
        pa, pb = _panels_per_group(a, n_own - rt), _panels_per_group(b, n_own - rt)
        assert pa < pb - (1.5 if rt == 32 else 0.0), (pa, pb)
    else:
        assert a == b


# ---- the one-GPU step's decisions (csrc/runtime/step.cpp, resolve_step_plan) ----------------
# Expected values: what the parent commit's own eligibility functions and tile builders return
# for each shape on 256 CUs with every toggle at its default (read off a host-only program linked
# against them, not reasoned out). Keys left out of a row are not pinned for that shape.
_LARGE = dict(small=False, small_fwd_fused=False, f8=False, q8=False, raw=True, fuse=True, half_c=True, dfold=True,
              keep_cos=True, bwd="fp16", forward_mfma="bf16", backward_mfma="fp16")
STEP_PLANS = {
    "headline": ((8192, 2048, "bf16", "fp16"), dict(_LARGE, n_fwd=528, n_own=528, n_dz=256)),
    "config2": ((8192, 512, "bf16", "fp16"), dict(_LARGE, n_fwd=528, n_own=528, n_dz=64)),
    "config4": ((2048, 8192, "bf16", "fp16"), dict(_LARGE, n_fwd=36, n_own=36, n_dz=256)),
    "config5-fp16": ((16384, 1024, "bf16", "fp16"), dict(_LARGE, n_fwd=2080, n_own=2080, n_dz=256)),
    "config5-fp8": ((16384, 1024, "bf16", "fp8"),
                    dict(_LARGE, f8=True, q8=True, raw=False, fuse=False, half_c=False, dfold=False,
                         forward_mfma="fp8", backward_mfma="fp8", n_fwd=2080, n_own=2080, n_dz=256)),
    "small-fused": ((512, 128, "bf16", "fp16"),
                    dict(small=True, small_fwd_fused=True, small_splits=8, f8=False, q8=False, raw=False, fuse=False,
                         half_c=False, dfold=False, bwd="fp16", forward_mfma="fp16", backward_mfma="fp16")),
    "small-prep": ((2048, 128, "bf16", "fp16"),
                   dict(small=True, small_fwd_fused=False, small_splits=8, raw=False, half_c=False, dfold=False)),
    "fp32": ((2048, 256, "fp32", "fp32"),
             dict(small=False, f8=False, q8=False, raw=False, fuse=False, half_c=False, dfold=False, bwd="fp32",
                  forward_mfma="fp32", backward_mfma="fp32", n_fwd=36, n_own=36, n_dz=8)),
    "dim-not-multiple-of-8": ((2500, 300, "bf16", "fp16"),
                              dict(small=False, f8=False, q8=False, raw=False, fuse=False, half_c=True, dfold=False,
                                   bwd="fp16", forward_mfma="fp16", backward_mfma="fp16", n_fwd=55, n_own=55,
                                   n_dz=20)),
}


@pytest.mark.parametrize("name", list(STEP_PLANS))
def test_step_plan_pins_the_decisions(C, name):
    (rows, dim, inp, comp), want = STEP_PLANS[name]
    plan = C.step_plan(rows, dim, inp, comp)
    assert {k: plan[k] for k in want} == want


def test_step_plan_follows_keep_cos_and_the_toggles(C):
    # recompute: no kept cosines, so neither the raw-operand forward nor half C
    plan = C.step_plan(8192, 2048, "bf16", "fp16", keep_cos=False)
    assert not plan["keep_cos"] and not plan["raw"] and not plan["half_c"] and plan["fuse"] and plan["dfold"]
    assert plan["forward_mfma"] == "fp16"
    # fp8 plans always keep their cosines
    assert C.step_plan(16384, 1024, "bf16", "fp8", keep_cos=False)["keep_cos"]
    # resolved per call: a toggle flipped between two calls shows in the next plan
    for get, put, key, args in [(C.half_c_enabled, C.set_half_c, "half_c", (8192, 2048, "bf16", "fp16")),
                                (C.raw_forward_enabled, C.set_raw_forward, "raw", (8192, 2048, "bf16", "fp16")),
                                (C.dot_fold_enabled, C.set_dot_fold, "dfold", (8192, 2048, "bf16", "fp16")),
                                (C.fp8_backward_enabled, C.set_fp8_backward, "q8", (16384, 1024, "bf16", "fp8")),
                                (C.small_path_enabled, C.set_small_path, "small", (512, 128, "bf16", "fp16"))]:
        old = get()
        try:
            put(False)
            assert not C.step_plan(*args)[key]
            put(True)
            assert C.step_plan(*args)[key]
        finally:
            put(old)


@pytest.mark.parametrize("rows,dim", [(8192, 2048), (2048, 8192), (16384, 1024), (8192, 512)])
def test_half_c_taken_at_every_shape_of_the_bitwise_test(C, rows, dim):
    """tests/test_gpu_half_c.py::test_half_c_gradient_bitwise_equal_to_full_c compares half C against
    the full C at these shapes; all four take half C, config 2's split-K dZ included (its pieces
    start at even K-steps: dz_half_c_eligible)."""
    assert C.step_plan(rows, dim, "bf16", "fp16")["half_c"]


@pytest.mark.parametrize("name", list(STEP_PLANS))
def test_bench_mfma_dtypes_agree_with_step_plan(C, monkeypatch, name):
    """bench.py labels its JSON with its own copy of the raw-forward / fp8-backward rules
    (mfma_dtypes). Run that code over a stand-in for the device-bound get_plan and compare with
    the dtypes the step actually resolves."""
    import argparse
    import types

    import torch

    import bench
    from ntxent_amd.ops import _ext

    (rows, dim, inp, comp), _ = STEP_PLANS[name]
    plan = C.step_plan(rows, dim, inp, comp)
    shim = types.SimpleNamespace(
        get_plan=lambda *a: types.SimpleNamespace(small=plan["small"], compute_dtype=comp, backward_dtype=plan["bwd"]),
        raw_forward_enabled=C.raw_forward_enabled, fp8_backward_enabled=C.fp8_backward_enabled)
    monkeypatch.setattr(_ext, "load", lambda *a, **k: shim)
    a = argparse.Namespace(dtype=inp, compute=comp, impl="fused", batch=rows // 2, dim=dim, temperature=0.07,
                           recompute=False)
    got = bench.mfma_dtypes(a, 1, 0, torch.device("cuda", 0))
    short = {k: v.split()[0].replace("e4m3", "fp8") for k, v in got.items()}
    assert short == {"forward": plan["forward_mfma"], "backward": plan["backward_mfma"]}
