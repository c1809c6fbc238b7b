#!/usr/bin/env python3
"""Digests of what the NT-Xent kernels compute, path by path, for checking a refactor bit for bit:
run this on two builds on the same machine, one process per build, and compare the lines.

  python tools/ntxent_digest.py     (loads the build of the checkout it lies in)

One line per case: SHA-256 (first 16 hex digits, as tools/xview_digest.py) of the raw bytes of the
loss, of dh, of the rows' LSE (log2 units, lse2[:rows]) and of the kept cosine tiles, for seeded
inputs built with a CPU torch.Generator (bf16 rows for the 16-bit and fp8 plans, fp32 rows for
fp32; the small-path cases name their rows' dtype). Every case first asserts, from the host planning bindings (as tests/test_gpu_probes.py),
that its shape takes the path it names on this machine's CU count, so a digest cannot silently
cover another kernel. The kept cosines of a case with a diagonal remainder are left out: that
launch writes the upper regions of its tiles only, the rest of the slot is not initialised.
"""
from __future__ import annotations

import hashlib
import math
import sys
from pathlib import Path

import torch

TAU_FX, TAU_MAX = 0.07, 0.02  # fixed-shift exponentials (2 log2(e) / tau < 120) / per-tile maxima


def digest(t: torch.Tensor) -> str:
    """tools/xview_digest.py's, over the bytes of any dtype (numpy has no bf16)."""
    return hashlib.sha256(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def rows(n_rows: int, d: int, seed: int, dtype) -> torch.Tensor:
    """Stacked views [n_rows, d]: two noisy copies of the same base rows."""
    g = torch.Generator().manual_seed(seed)
    n = n_rows // 2
    base = torch.randn(n, d, generator=g)
    return torch.cat([base + 0.3 * torch.randn(n, d, generator=g), base + 0.3 * torch.randn(n, d, generator=g)], 0).to(dtype)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("ntxent_digest: needs a GPU (no CPU fall-back: the digests are the kernels')")
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import ntxent_amd
    from ntxent_amd.ops import _ext
    from ntxent_amd.parallel import emulate

    C = _ext.load(build_if_missing=False)
    print(f"# build {C.__file__}")
    dev = torch.device("cuda", 0)
    cus = C.device_info(0)["num_cus"]
    TORCH = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
    in_name = lambda comp: "fp32" if comp == "fp32" else "bf16"  # the rows' dtype unless a case names one
    assert 2 * math.log2(math.e) / TAU_FX < 120 <= 2 * math.log2(math.e) / TAU_MAX

    def plan(n, d, comp, keep=True, inp=None):
        """(step plan, forward K-steps per tile, row tiles) as the op resolves them."""
        p = C.step_plan(n, d, inp or in_name(comp), comp, keep, cus)
        g = C.geometry(n, d)
        return p, g["dim_k"] * (4 if comp == "fp32" else 2) // C.K_STEP_BYTES, g["row_tiles"]

    def step(tag, n, d, comp, tau=TAU_FX, keep=True, cosines=True, inp=None):
        h = rows(n, d, 1000 * n + d, TORCH[inp or in_name(comp)]).to(dev)
        loss, zq, zqt, inv, lse2, sc, cpos = C.fused_forward(h, tau, comp, keep)
        dh = C.fused_backward(h, zq, zqt, inv, lse2, sc if keep else None, cpos, torch.ones(1, device=dev), tau)
        torch.cuda.synchronize()
        line = f"{tag} {n}x{d} {comp} tau={tau}: loss {digest(loss)} dh {digest(dh)} lse {digest(lse2[:n])}"
        if sc is not None and cosines:
            line += f" cos {digest(sc)}"
        print(line, flush=True)

    # ---- the small path: fused and separate row prologue ------------------------------------------
    # (16-bit plans only: fp32 compute has no small path; fp32, fp16 and bf16 rows in)
    for inp, comp in (("fp32", "fp16"), ("fp16", "fp16"), ("bf16", "fp16"), ("bf16", "bf16")):
        for n, d, fuse_rows, fused in ((600, 200, -1, True), (600, 200, 0, False), (1500, 96, -1, False)):
            C.set_small_fuse_rows(fuse_rows)
            try:
                p, _, _ = plan(n, d, comp, inp=inp)
                assert p["small"] and p["small_fwd_fused"] == fused, (n, d, inp, comp, p)
                step(f"small fused={int(fused)} rows={inp}", n, d, comp, inp=inp)
            finally:
                C.set_small_fuse_rows(-1)
    # ---- the large pipeline at small size: kept cosines and the recompute (coefficient GEMM) -----
    C.set_small_path(False)
    try:
        for comp in ("fp32", "fp16", "bf16"):
            for n, d in ((600, 320), (600, 300)):
                for keep in (True, False):
                    p, _, _ = plan(n, d, comp, keep)
                    assert not p["small"] and not p["raw"] and p["keep_cos"] == keep, (n, d, comp, p)
                    step("large keep" if keep else "large recompute", n, d, comp, keep=keep)
    finally:
        C.set_small_path(True)
    # ---- split-K forward with padded rows, both exponential forms --------------------------------
    for comp, n, d in (("fp16", 1000, 2048), ("bf16", 1000, 2048), ("fp32", 1000, 1024)):
        p, nk, rt = plan(n, d, comp)
        assert not p["small"] and C.fwd_splitk_pieces(p["n_own"], nk, cus, rt) >= 2, (n, d, comp)
        for tau in (TAU_FX, TAU_MAX):
            step("splitk-fwd", n, d, comp, tau)
    # ---- diagonal remainder with a padded last tile ----------------------------------------------
    for comp in ("fp32", "fp16", "bf16"):
        p, nk, rt = plan(5800, 256, comp)
        assert C.fwd_diag_remainder(p["n_own"], nk, cus, rt) > 0 and not p["raw"], comp
        for tau in (TAU_FX, TAU_MAX):
            step("diag-remainder", 5800, 256, comp, tau, cosines=False)
    # ---- stream-K remainder ----------------------------------------------------------------------
    for comp in ("fp32", "fp16"):
        p, nk, rt = plan(6144, 2048, comp)
        s = C.schedule(p["n_own"], nk, cus)
        assert C.fwd_diag_remainder(p["n_own"], nk, cus, rt) == 0 and C.fwd_splitk_pieces(p["n_own"], nk, cus, rt) == 0
        assert s["sk_tiles"] > 0 and s["dp_tiles"] > 0 and s["ipb"] < nk
        step("stream-k", 6144, 2048, comp)
    # ---- 8192 x 256: raw forward, LSE fold, half C, split-K dZ -----------------------------------
    for comp in ("fp16", "bf16"):
        p, nk, rt = plan(8192, 256, comp)
        assert p["raw"] and p["half_c"] and p["dfold"] and p["fuse"], p
        assert C.lse_fold_enabled() and C.fwd_diag_remainder(p["n_own"], nk, cus, rt) * 256 == 8192 // 2
        assert C.fwd_splitk_pieces(p["n_dz"], 8192 * 2 // C.K_STEP_BYTES, cus, 1) >= 3
        step("raw+fold+halfC", 8192, 256, comp, cosines=False)
    # ---- fp8 forward with the e4m3 backward (smallest shape of tests/test_gpu_fp8bwd.py) ---------
    p, _, _ = plan(3000, 256, "fp8")
    assert p["f8"] and p["q8"] and C.fp8_backward_enabled(), p
    step("fp8+e4m3-bwd", 3000, 256, "fp8", 0.1, cosines=False)
    # ---- positive rank ---------------------------------------------------------------------------
    for n, d in ((600, 200), (1000, 2048)):
        for comp in ("fp32", "fp16", "bf16"):
            rank, pos, hard = ntxent_amd.positive_rank(rows(n, d, 1000 * n + d, torch.float32).to(dev), compute=comp)
            print(f"pos_rank {n}x{d} {comp}: rank {digest(rank)} pos_cos {digest(pos)} hard_neg_cos {digest(hard)}")
    # ---- emulated ranks: cross tiles and the mirrored partner coefficients ------------------------
    drivers = {"dist": emulate.emulated_dist_forward_backward, "sym": emulate.emulated_sym_forward_backward}
    for W in (2, 3):
        for comp in ("fp32", "fp16"):
            plans = [C.get_plan(300, 320, W, r, TAU_FX, comp, 0) for r in range(W)]
            assert all(q.world == W and not q.small and q.rows_pad > q.rows and q.col_tiles == W * q.row_tiles for q in plans)
            shards = [rows(300, 320, 7000 + 101 * r + W, torch.float32).to(dev) for r in range(W)]
            for name, drv in drivers.items():
                loss, grads = drv(shards, TAU_FX, compute=comp)
                torch.cuda.synchronize()
                print(f"emulated-{name} W={W} 300x320 {comp}: loss {digest(loss)} " +
                      " ".join(f"dh{r} {digest(g)}" for r, g in enumerate(grads)), flush=True)


if __name__ == "__main__":
    main()
