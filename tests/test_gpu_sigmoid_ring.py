"""``exchange="ring"`` of the distributed pairwise sigmoid loss (parallel/sigmoid.py, the block form of the
xview_sigmoid_* kernels and the accumulating xview_dz_kernel) on an MI355X: W virtual ranks through
the emulation, which hands every rank the other ranks' rows one slot at a time in ring order, and W
real processes on the one GPU over gloo and RCCL, against the fp64 oracle ``reference.sigmoid_loss`` on
the global batch in pair order and against the gather path on the same shards.

The bounds are test_gpu_sigmoid_dist's: per quantity 2 x max(test_gpu_sigmoid.TABLE[compute], the error
the one-GPU sigmoid_loss shows on the same global batch in the same run); the exact cases take
test_gpu_sigmoid._fp32_bound. The loss and dL/dbias are bitwise the gather path's (every tile's partial
lies at the same place of the same fixed-order sums); dh and dL/dtau are sums over the blocks in ring
order, not slot order, and are held to the bound. Every gradient is taken at grad_out = 0.7.

Largest errors measured on MI355X over the parity shapes below (loss / dh / dtau / dbias): fp32 6.8e-8 /
1.5e-6 / 7.4e-8 / 1.1e-7, fp16 1.9e-7 / 1.0e-3 / 2.1e-5 / 1.5e-7, bf16 6.8e-7 / 4.9e-3 / 3.1e-5 / 8.5e-7; the
one-GPU sigmoid_loss on the same global batches in the same run: fp32 6.8e-8 / 2.6e-6 / 7.4e-8 / 1.1e-7, fp16
the same four but dbias 1.3e-7, bf16 the same four (profiles/sigmoid_ring/parity.log). Ring against gather:
loss and dL/dbias the same bits in every case, dh at most 2.4e-6 of the global max|g| apart, dL/dtau the
same fp32 number in every case. Largest probe-row errors 6.8e-7 (fp32), 3.5e-4 (fp16), 3.2e-3 (bf16). Peak
bytes of rank 0's stage forward + backward (fp16, n = 200, d = 100): ring 919 552 at W = 2 and at W = 8,
gather 1 312 768 and 3 672 064.
"""
import functools
import math
import os

import pytest
import torch
import torch.multiprocessing as mp

import ntxent_amd
from ntxent_amd.ops import _ext
from ntxent_amd.ops import reference as R
from test_gpu_sigmoid import PAIRS, _errors, _fmt, _fp32_bound, _oracle, _softplus, _t
from test_gpu_sigmoid_dist import (CASES, GO, PROBE_BIAS, PROBE_T, PROC_BIAS, PROC_T, _bound, _case, _emulate,
                                   _free_port, _join, _probe_oracle, _shards, _split)
from test_infonce_dist_cpu import PROBE_SHAPES

pytestmark = pytest.mark.gpu


def _ring(shards, T, bias, compute, go=GO, **kw):
    return _emulate(shards, T, bias, compute, go=go, exchange="ring", **kw)


@functools.lru_cache(maxsize=None)
def _both(W, n, d, compute, T, bias):
    """(ring, gather) emulations of one case, and the case: computed once, shared, left unchanged."""
    shards, hg, ref = _case(W, n, d, T, bias)
    return _ring(shards, T, bias, compute), _emulate(shards, T, bias, compute), hg, ref


# ---- 1. emulated parity with the fp64 oracle on the global batch ----------------------------------------
@pytest.mark.parametrize("T,bias", PAIRS)
@pytest.mark.parametrize("W,n,d,compute", CASES)
def test_ring_parity_with_the_oracle(gpu, W, n, d, compute, T, bias):
    (loss, grads, dtau, dbias), _, hg, ref = _both(W, n, d, compute, T, bias)
    e_new = _errors((loss, _join(grads), dtau, dbias), ref)
    bound, e_old = _bound(hg, T, bias, compute, ref)
    print(f"SIGDIST W={W} n={n} d={d} compute={compute} tau={T} bias={bias} dist loss/dh/dtau/dbias={_fmt(e_new)} "
          f"one-GPU={_fmt(e_old)} bound={_fmt(bound)}")
    assert all(math.isfinite(e) for e in e_new)
    assert all(e <= b for e, b in zip(e_new, bound)), (e_new, bound)


# ---- 2. bitwise ties to the gather path -------------------------------------------------------------------
@pytest.mark.parametrize("T,bias", PAIRS)
@pytest.mark.parametrize("W,n,d,compute", CASES)
def test_ring_ties_to_the_gather_path(gpu, W, n, d, compute, T, bias):
    """Same shards, same compute: the loss and dL/dbias are the same bits (the tiles' partials lie at
    the same places of the same sums); dh and dL/dtau, summed in block order, stay within the bound of
    the oracle parity of each other."""
    ring, gather, hg, ref = _both(W, n, d, compute, T, bias)
    assert torch.equal(ring[0], gather[0]), (ring[0].item(), gather[0].item())
    assert torch.equal(ring[3], gather[3]), (ring[3].item(), gather[3].item())
    bound, _ = _bound(hg, T, bias, compute, ref)
    gr, gg = _join(ring[1]).double(), _join(gather[1]).double()
    dh_diff = (gr - gg).abs().max().item() / ref[1].abs().max().item()
    tau_diff = abs(ring[2].item() - gather[2].item()) / max(abs(ref[2]), 1e-300)
    print(f"SIGRINGTIE W={W} n={n} d={d} compute={compute} tau={T} bias={bias} dh_diff={dh_diff:.3e} "
          f"dtau_diff={tau_diff:.3e} bound={_fmt(bound)}")
    assert dh_diff <= bound[1] and tau_diff <= bound[2]


# ---- 3. exact cases -----------------------------------------------------------------------------------
@pytest.mark.parametrize("T,bias", PAIRS)
@pytest.mark.parametrize("compute", ["fp32", "fp16", "bf16"])
def test_identical_rows(gpu, compute, T, bias):
    """test_gpu_sigmoid_dist.test_identical_rows through the ring: every cosine is 1."""
    W, n = 3, 37
    N = W * n
    row = torch.zeros(40)
    row[:16] = 2.0 * torch.tensor([1, -1, 1, 1, -1, 1, -1, -1, 1, 1, -1, 1, 1, -1, -1, 1])
    hg = row.repeat(2 * N, 1).cuda()
    loss, grads, _, _ = _ring(_split(hg, W), T, bias, compute)
    x = 1.0 / T + bias
    want = _softplus(-x) + (N - 1) * _softplus(x)
    bound = _fp32_bound(hg, T, bias)
    le = abs(loss.item() - want) / max(1.0, want)
    print(f"SIGRINGEXACT identical W={W} n={n} compute={compute} tau={T} bias={bias} loss_err={le:.3e} bound={bound[0]:.3e}")
    assert le <= bound[0], (loss.item(), want)
    assert all(torch.isfinite(g).all() for g in grads)


@pytest.mark.parametrize("T,bias", PAIRS)
@pytest.mark.parametrize("compute", ["fp32", "fp16", "bf16"])
def test_orthogonal_rows(gpu, compute, T, bias):
    """Global one-hot rows 3 eye(N): exact in every dtype, every negative has cos = 0."""
    W, n = 2, 37
    N = W * n
    v = 3.0 * torch.eye(N, (N + 63) // 64 * 64)
    hg = torch.cat([v, v], 0).cuda()
    loss, grads, _, _ = _ring(_split(hg, W), T, bias, compute)
    want = _softplus(-(1.0 / T + bias)) + (N - 1) * _softplus(bias)
    gref = GO * _oracle(hg, T, bias)[1]
    bound = _fp32_bound(hg, T, bias)
    le = abs(loss.item() - want) / max(1.0, want)
    ge = (_join(grads).double() - gref).abs().max().item() / gref.abs().max().item()
    print(f"SIGRINGEXACT orthogonal W={W} n={n} compute={compute} tau={T} bias={bias} loss_err={le:.3e} "
          f"bound={bound[0]:.3e} dh_err={ge:.3e} bound={bound[1]:.3e}")
    assert le <= bound[0], (loss.item(), want)
    assert ge <= bound[1]


# ---- 4. planted-pair probes -----------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("W,rows", PROBE_SHAPES)
def test_planted_pair_probes(gpu, W, rows, compute):
    """test_gpu_sigmoid_dist.test_planted_pair_probes's inputs and assertions through the ring: a pair
    taken from the wrong block, a positive tested against the buffer's place instead of the slot's
    identity, or a block stored over the slab instead of added to it, moves a probe row by at least
    sig_min of the global max|g|."""
    hg, ref, sig_min, probes, labels = _probe_oracle(W, rows)
    loss, grads, dtau, dbias = _ring(_split(hg, W), PROBE_T, PROBE_BIAS, compute)
    g = _join(grads)
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    bound, _ = _bound(hg, PROBE_T, PROBE_BIAS, compute, ref)
    idx = torch.tensor(probes, device=g.device)
    rerr = (g[idx].double() - ref[1][idx]).abs().amax(2) / ref[1].abs().max()
    e_new = _errors((loss, g, dtau, dbias), ref)
    k = rerr.amax(1).argmax().item()
    print(f"PROBE sigmoid-ring W={W} rows={rows} compute={compute} probes={len(probes)} sig_min={sig_min:.3f} "
          f"row_err_max={rerr.max().item():.3e} at={probes[k]}{'/'.join(labels[k])} cap={sig_min / 4:.3e} "
          f"loss/dh/dtau/dbias={_fmt(e_new)} bound={_fmt(bound)}")
    assert sig_min >= 0.2, sig_min
    assert bound[1] <= sig_min / 4, (bound[1], sig_min)
    bad = [(probes[i], labels[i], [f"{e:.2e}" for e in rerr[i].tolist()]) for i in range(len(probes))
           if rerr[i].max().item() > bound[1]]
    assert not bad, f"probe rows over the dh bound {bound[1]:.2e}: {bad}"
    assert e_new[0] <= bound[0] and e_new[2] <= bound[2] and e_new[3] <= bound[3], (e_new, bound)


# ---- 5. scalar gradients, repeatability and block order ------------------------------------------------
@pytest.mark.parametrize("W,n,d,compute", [(3, 129, 160, "fp16"), (2, 37, 40, "fp32")])
def test_dh_does_not_depend_on_the_scalar_gradients(gpu, W, n, d, compute):
    both, _, _, _ = _both(W, n, d, compute, 0.1, -10.0)
    shards, _, _ = _case(W, n, d, 0.1, -10.0)
    for want_tau, want_bias in [(False, False), (True, False), (False, True)]:
        got = _ring(shards, 0.1, -10.0, compute, want_tau=want_tau, want_bias=want_bias)
        assert torch.equal(got[0], both[0]) and all(torch.equal(a, b) for a, b in zip(got[1], both[1]))
        assert (got[2] is None) == (not want_tau) and (got[3] is None) == (not want_bias)
        assert got[2] is None or torch.equal(got[2], both[2])
        assert got[3] is None or torch.equal(got[3], both[3])


@pytest.mark.parametrize("W,n,d,compute", [(3, 129, 160, "fp16"), (2, 200, 100, "bf16")])
def test_two_runs_are_bitwise_equal(gpu, W, n, d, compute):
    a, _, _, _ = _both(W, n, d, compute, 0.1, -10.0)
    b = _ring(_case(W, n, d, 0.1, -10.0)[0], 0.1, -10.0, compute)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("compute", ["fp32", "fp16"])
@pytest.mark.parametrize("T,bias", PAIRS)
def test_every_rank_is_within_the_bound(gpu, compute, T, bias):
    """Each rank starts its ring at another block (r: r, r-1, r-2): the first block stores the slab and
    the others add to it, so every rank's rows are held to the bound on their own, not their join."""
    W, n, d = 3, 129, 160
    (_, grads, _, _), _, hg, ref = _both(W, n, d, compute, T, bias)
    bound, _ = _bound(hg, T, bias, compute, ref)
    gmax = ref[1].abs().max().item()
    for r, want in enumerate(_split(ref[1], W)):
        e = (grads[r].double() - want).abs().max().item() / gmax
        print(f"SIGRINGRANK W={W} n={n} d={d} compute={compute} tau={T} bias={bias} rank={r} dh_err={e:.3e} bound={bound[1]:.3e}")
        assert e <= bound[1], (r, e, bound[1])


# ---- 6. memory does not grow with W ---------------------------------------------------------------------
def _stage_peak(W, exchange):
    """Peak bytes above the entry level around rank 0's stage forward plus backward (fp16, n = 200,
    d = 100), every rank's prep outputs built before."""
    from ntxent_amd.parallel.infonce import _CDT, xview_compute
    from ntxent_amd.parallel.sigmoid import (sigmoid_ring_stage_backward, sigmoid_ring_stage_forward,
                                             sigmoid_stage_forward)

    C = _ext.load()
    n, d, T, bias = 200, 100, 0.1, -10.0
    hs = _shards(W, n, d)
    dev = hs[0].device
    comp = xview_compute(hs[0].dtype, False, "fp16")
    plans = [C.get_plan(2 * n, d, W, r, T, comp, dev.index) for r in range(W)]
    Rpad = plans[0].rows_pad
    go = torch.tensor([GO], dtype=torch.float32, device=dev)
    if exchange == "ring":
        preps = [C.prep(hs[r], plans[r]) for r in range(W)]
        zqs = [p[0] for p in preps]

        def visit(fn):
            for s in range(W):
                fn((0 - s) % W, zqs[(0 - s) % W], 0)
    else:
        zq_all = torch.empty((W * Rpad, plans[0].ld_k), dtype=_CDT[comp], device=dev)
        preps = [C.prep(hs[r], plans[r], zq_all[r * Rpad:(r + 1) * Rpad], None) for r in range(W)]
    inv = preps[0][1]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    if exchange == "ring":
        share = sigmoid_ring_stage_forward(C, plans[0], zqs[0], hs[0], inv, bias, visit)
        dh, shares = sigmoid_ring_stage_backward(C, plans[0], zqs[0], hs[0], inv, bias, go, True, True, visit)
    else:
        share = sigmoid_stage_forward(C, plans[0], zq_all, hs[0], inv, bias)
        dh, shares = C.xview_sigmoid_dist_backward(hs[0], zq_all, inv, go, plans[0], bias, True, True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert torch.isfinite(share) and torch.isfinite(dh).all() and torch.isfinite(shares).all()
    return peak, plans[0]


def test_ring_memory_does_not_grow_with_the_world(gpu):
    """The ring's stage buffers do not depend on W but for lpart (8 B) and bias_part (16 B) per tile,
    nT^2 W tiles: from W = 2 to W = 8 they grow by 6 nT^2 (8 + 16) bytes, and 64 KiB are allowed for the
    allocator's rounding. The gather stage ops' coefficient block and zt alone grow by more than 2 MiB
    over the same step."""
    ring2, plan = _stage_peak(2, "ring")
    ring8, _ = _stage_peak(8, "ring")
    gather2, _ = _stage_peak(2, "gather")
    gather8, _ = _stage_peak(8, "gather")
    nT = (200 + 127) // 128
    growth = 6 * nT * nT * (8 + 16)
    print(f"SIGRINGMEM fp16 n=200 d=100 peak bytes ring W=2 {ring2} W=8 {ring8} gather W=2 {gather2} W=8 {gather8} "
          f"allowed growth {growth} + 65536")
    assert ring8 - ring2 <= growth + 64 * 1024, (ring2, ring8)
    assert ring8 < gather8, (ring8, gather8)
    assert gather8 - gather2 > 2 * 1024 * 1024, (gather2, gather8)  # what the ring is for


# ---- 7. real processes on the one GPU ---------------------------------------------------------------------
def _worker(rank, W, port, n, d, compute, backend, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    if backend == "nccl":
        from ntxent_amd.parallel.commstats import rccl_shared_gpu_env

        rccl_shared_gpu_env(rank)
        dist.init_process_group("nccl", rank=rank, world_size=W, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=W)
    try:
        from ntxent_amd.parallel import dist_sigmoid_loss

        go = torch.tensor(GO, device="cuda")

        def step(tau, bias, exchange="ring"):
            h = _shards(W, n, d)[rank].requires_grad_(True)
            loss = dist_sigmoid_loss(h, tau, bias, compute=compute, exchange=exchange)
            leaves = [v for v in (tau, bias) if isinstance(v, torch.Tensor)]
            grads = torch.autograd.grad(loss, [h] + leaves, go)
            torch.cuda.synchronize()
            return loss, grads

        loss, (g, dtau, dbias) = step(_t(PROC_T), _t(PROC_BIAS))
        # float arguments (a backward that does not communicate) and one tensor alone: the same loss and dh
        same = True
        for tau, bias in ((PROC_T, PROC_BIAS), (_t(PROC_T), PROC_BIAS), (PROC_T, _t(PROC_BIAS))):
            l2, g2 = step(tau, bias)
            same = same and torch.equal(l2, loss) and torch.equal(g2[0], g)
            if len(g2) == 2:
                same = same and torch.equal(g2[1], dtau if isinstance(tau, torch.Tensor) else dbias)
        gather_loss, _ = step(PROC_T, PROC_BIAS, exchange="gather")
        q.put((rank, loss.item(), g.cpu().numpy(), dtau.item(), dbias.item(), same, gather_loss.item()))  # by value
    except Exception as e:  # surface the failure in the parent
        q.put((rank, repr(e), None, None, None, False, None))
    finally:
        dist.destroy_process_group()


def _run_and_check(W, n, d, compute, backend):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, W, port, n, d, compute, backend, q)) for r in range(W)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(W):
        r, *rest = q.get(timeout=240)
        res[r] = rest
    for p in procs:
        p.join(timeout=60)
    for r, (loss, g, *_) in res.items():
        assert g is not None, f"rank {r} failed: {loss}"
    shards, hg, ref = _case(W, n, d, PROC_T, PROC_BIAS)
    eloss, egrads, etau, ebias = _ring(shards, PROC_T, PROC_BIAS, compute)
    bound, _ = _bound(hg, PROC_T, PROC_BIAS, compute, ref)
    for r in range(W):
        loss, g, dtau, dbias, same, gather_loss = res[r]
        assert same, f"rank {r}: float or single-tensor arguments change the loss, dh or a scalar gradient"
        assert (loss, dtau, dbias) == tuple(res[0][i] for i in (0, 2, 3))  # identical on all ranks
        for got, emu in ((loss, eloss), (dtau, etau), (dbias, ebias)):  # (the all-reduce order may differ)
            assert abs(got - emu.item()) <= 1e-6 * abs(emu.item()), (r, got, emu.item())
        assert loss == gather_loss, (r, loss, gather_loss)  # the same shares through the same all-reduce
        assert torch.equal(torch.from_numpy(g), egrads[r].cpu()), f"rank {r}: gradient differs from the emulation's"
    dev = hg.device
    e = _errors((torch.tensor(res[0][0]), _join([torch.from_numpy(res[r][1]) for r in range(W)]).to(dev),
                 torch.tensor(res[0][2]), torch.tensor(res[0][3])), ref)
    print(f"SIGRINGPROC {backend} W={W} n={n} d={d} compute={compute} loss/dh/dtau/dbias={_fmt(e)} bound={_fmt(bound)}")
    assert all(x <= b for x, b in zip(e, bound)), (e, bound)


def test_multiprocess_gloo(gpu):
    _run_and_check(2, 150, 100, "fp16", "gloo")


def test_multiprocess_rccl(gpu):
    _run_and_check(3, 129, 160, "fp32", "nccl")


# ---- 8. no disturbance ------------------------------------------------------------------------------------
def test_does_not_disturb_sigmoid_loss_or_the_gather_path(gpu):
    """A ring step between sigmoid_loss's forward and backward changes neither, and the gather
    emulation returns the same bits before and after a ring step."""
    from test_gpu_sigmoid import _inputs

    h = _inputs(1024, 256, torch.bfloat16, seed=9)
    shards = _shards(2, 200, 100)
    gather_before = _emulate(shards, 0.1, -10.0, "fp16")
    alone = _ring(shards, 0.1, -10.0, "fp16")

    def run(between):
        x = h.clone().requires_grad_(True)
        loss = ntxent_amd.sigmoid_loss(x, 0.1, -10.0)
        got = _ring(shards, 0.1, -10.0, "fp16") if between else None
        loss.backward()
        return loss.detach().clone(), x.grad.clone(), got

    l0, g0, _ = run(False)
    l1, g1, got = run(True)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    assert torch.equal(got[0], alone[0]) and all(torch.equal(a, b) for a, b in zip(got[1], alone[1]))
    assert torch.equal(got[2], alone[2]) and torch.equal(got[3], alone[3])
    gather_after = _emulate(shards, 0.1, -10.0, "fp16")
    assert torch.equal(gather_before[0], gather_after[0]) and torch.equal(gather_before[2], gather_after[2])
    assert torch.equal(gather_before[3], gather_after[3])
    assert all(torch.equal(a, b) for a, b in zip(gather_before[1], gather_after[1]))
