"""Distributed cross-view InfoNCE (parallel/infonce.py, the xview_dist_* kernels of
csrc/kernels/xview_kernels.hip) on an MI355X: W virtual ranks through the emulation, and W real
processes on the one GPU over gloo and RCCL, against the fp64 oracle on the global batch in pair order.

Bounds come from the project, not from the code under test: for the loss (relative, floor 1) and for
dh (max-abs over the global max|g|), 2 x max(test_gpu_infonce.TABLE[compute], the error the one-GPU
info_nce_loss shows on the same global batch against the same oracle, same compute, same run). The
exact cases take test_gpu_infonce._fp32_bound's rule on the global batch in every compute dtype, the
probes 2 x test_gpu_probes.ROW_MEASURED per probe row (asserted to be under sig_min / 4).
"""
import functools
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

import ntxent_amd
from ntxent_amd.ops import reference as R
from test_gpu_infonce import TABLE, _fp32_bound, _inputs
from test_gpu_probes import ROW_MEASURED
from test_infonce_dist_cpu import PROBE_SHAPES, dist_probe_case
from test_probes_cpu import row_errors

pytestmark = pytest.mark.gpu

T = 0.07
GO = 0.7


def _shards(W, n, d):
    return [_inputs(2 * n, d, torch.float32, seed=n + d + 101 * r)[1] for r in range(W)]


def _split(hg, W):
    """The rank shards [a_r; b_r] of a global batch in pair order."""
    N = hg.shape[0] // 2
    n = N // W
    return [torch.cat([hg[r * n:(r + 1) * n], hg[N + r * n:N + (r + 1) * n]], 0).contiguous() for r in range(W)]


def _join(grads):
    n = grads[0].shape[0] // 2
    return torch.cat([g[:n] for g in grads] + [g[n:] for g in grads], 0)


def _oracle(hg, temperature=T):
    """(loss, GO x dh) of the fp64 oracle on the device rows cast to double."""
    x = hg.detach().double().requires_grad_(True)
    loss = R.info_nce_loss(x, temperature)
    (g,) = torch.autograd.grad(loss, x)
    return loss.item(), GO * g


def _errors(loss, grad, ref):
    lref, gref = ref
    return (abs(loss - lref) / max(1.0, abs(lref)),
            (grad.double() - gref).abs().max().item() / max(gref.abs().max().item(), 1e-300))


def _one_gpu(hg, compute, temperature=T):
    x = hg.clone().requires_grad_(True)
    loss = ntxent_amd.info_nce_loss(x, temperature, compute=compute)
    (g,) = torch.autograd.grad(loss, x, torch.tensor(GO, device=x.device))
    return loss.item(), g


def _bound(hg, ref, compute):
    """Group 1's bound on this global batch, and the one-GPU errors it was taken from."""
    e_old = _errors(*_one_gpu(hg, compute), ref)
    return tuple(2.0 * max(t, e) for t, e in zip(TABLE[compute][:2], e_old)), e_old


def _emulate(shards, compute, temperature=T):
    from ntxent_amd.parallel.emulate import emulated_xview_forward_backward

    loss, grads = emulated_xview_forward_backward(shards, temperature, compute=compute, grad_out=GO)
    torch.cuda.synchronize()
    return loss.item(), grads


# ---- 1. emulated parity with the fp64 oracle on the global batch ----------------------------------------
CASES = [(2, 37, 40, "fp32"), (3, 129, 160, "fp32"), (3, 129, 160, "fp16"), (2, 200, 100, "bf16"),
         (4, 128, 64, "fp32"), (8, 37, 40, "fp16"),
         # world 1: the stage ops as the one-GPU op rides on them (a second tile of one valid row,
         # three fp16 K-steps)
         (1, 129, 160, "fp16"), (1, 37, 40, "fp32")]


@functools.lru_cache(maxsize=None)
def _case(W, n, d):
    shards = _shards(W, n, d)
    hg = R.global_pair_order(shards)
    return shards, hg, _oracle(hg)


@pytest.mark.parametrize("W,n,d,compute", CASES)
def test_emulated_parity_with_the_oracle(gpu, W, n, d, compute):
    shards, hg, ref = _case(W, n, d)
    loss, grads = _emulate(shards, compute)
    e_new = _errors(loss, _join(grads), ref)
    bound, e_old = _bound(hg, ref, compute)
    print(f"XVDIST W={W} n={n} d={d} compute={compute} dist loss/dh={e_new[0]:.3e}/{e_new[1]:.3e} "
          f"one-GPU={e_old[0]:.3e}/{e_old[1]:.3e} bound={bound[0]:.3e}/{bound[1]:.3e}")
    assert math.isfinite(loss) and all(torch.isfinite(g).all() for g in grads)
    assert e_new[0] <= bound[0] and e_new[1] <= bound[1], (e_new, bound)


# ---- 2. exact cases -----------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["fp32", "fp16", "bf16"])
def test_identical_rows(gpu, compute):
    """Every cosine is 1: the loss is log(W n); a counted pad column or slot gap gives another number."""
    W, n, d = 3, 37, 40
    row = torch.randn(d, generator=torch.Generator().manual_seed(1))
    hg = row.repeat(2 * W * n, 1).cuda()
    loss, grads = _emulate(_split(hg, W), compute)
    lt, _ = _fp32_bound(hg, T)
    want = math.log(W * n)
    err = abs(loss - want) / want
    worst = max((g.abs().max(1).values * row.norm().item()).max().item() for g in grads)
    print(f"XVDISTEXACT identical W={W} n={n} compute={compute} loss_rel_err={err:.3e} bound={lt:.3e} dh*|h|={worst:.3e}")
    assert err <= lt, (loss, want, lt)
    assert worst <= 1e-6


@pytest.mark.parametrize("compute", ["fp32", "fp16", "bf16"])
def test_orthogonal_rows(gpu, compute):
    """Global one-hot rows 3 eye(N) at tau 0.5: exact in every dtype, the fp32 tolerance for all."""
    W, n = 2, 37
    N = W * n
    v = 3.0 * torch.eye(N, (N + 63) // 64 * 64)
    hg = torch.cat([v, v], 0).cuda()
    loss, grads = _emulate(_split(hg, W), compute, 0.5)
    want = math.log1p((N - 1) * math.exp(-2.0))
    _, gref = _oracle(hg, 0.5)
    lt, gt = _fp32_bound(hg, 0.5)
    le = abs(loss - want) / max(1.0, want)
    ge = (_join(grads).double() - gref).abs().max().item() / gref.abs().max().item()
    print(f"XVDISTEXACT orthogonal W={W} n={n} compute={compute} loss_rel_err={le:.3e} bound={lt:.3e} "
          f"dh_rel_err={ge:.3e} bound={gt:.3e}")
    assert le <= lt, (loss, want)
    assert ge <= gt


# ---- 3. planted-pair probes -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _probe_oracle(W, rows):
    h64, probes, labels = dist_probe_case(W, rows)
    hg = h64.float().cuda()
    x = hg.double().requires_grad_(True)
    loss = R.info_nce_loss(x, T)
    (g,) = torch.autograd.grad(loss, x)
    sig, p_ij = R.probe_signatures(x.detach(), T, probes, grad=g, cross_view=True)
    assert sig.min().item() >= 0.2 and 0.15 <= p_ij.min().item() and p_ij.max().item() <= 0.85
    return hg, (loss.item(), GO * g), sig.min().item(), probes, labels


@pytest.mark.parametrize("compute", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("W,rows", PROBE_SHAPES)
def test_planted_pair_probes(gpu, W, rows, compute):
    """Cross-view probes in every rank's own block and across ranks (the other rank's would-be
    positive, its neighbours, the last and first valid columns of a slot), each carrying at least
    sig_min of two rows' gradients: rows per rank 300 (n = 150: a padded second tile) and 258 (n = 129)."""
    hg, ref, sig_min, probes, labels = _probe_oracle(W, rows)
    loss, grads = _emulate(_split(hg, W), compute)
    g = _join(grads)
    assert math.isfinite(loss) and torch.isfinite(g).all()
    rerr = row_errors(g, ref[1], probes)
    e_new = _errors(loss, g, ref)
    (lt, gt), _ = _bound(hg, ref, compute)
    bound = 2.0 * ROW_MEASURED[compute]
    k = rerr.amax(1).argmax().item()
    print(f"PROBE xview-dist W={W} rows={rows} compute={compute} probes={len(probes)} sig_min={sig_min:.3f} "
          f"row_err_max={rerr.max().item():.3e} at={probes[k]}{'/'.join(labels[k])} bound={bound:.3e} cap={sig_min / 4:.3e} "
          f"loss_err={e_new[0]:.3e} (bound {lt:.1e}) grad_err={e_new[1]:.3e} (bound {gt:.1e})")
    assert bound <= sig_min / 4, (bound, sig_min)
    bad = [(probes[i], labels[i], [f"{e:.2e}" for e in rerr[i].tolist()]) for i in range(len(probes))
           if rerr[i].max().item() > bound]
    assert not bad, f"probe rows over the per-row bound {bound:.2e}: {bad}"
    assert e_new[0] <= lt and e_new[1] <= gt, (e_new, lt, gt)


# ---- 4. real processes on the one GPU ---------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


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
        from ntxent_amd.parallel import dist_info_nce_loss

        out = []
        for overlap in (True, False):
            h = _shards(W, n, d)[rank].requires_grad_(True)
            loss = dist_info_nce_loss(h, T, compute=compute, overlap=overlap)
            (g,) = torch.autograd.grad(loss, h, torch.tensor(GO, device=h.device))
            torch.cuda.synchronize()
            out.append((loss, g))
        same = torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        q.put((rank, out[0][0].item(), out[0][1].cpu().numpy(), same))  # by value: no shared-memory fd hand-off
    except Exception as e:  # surface the failure in the parent
        q.put((rank, repr(e), None, False))
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
        r, loss, g, same = q.get(timeout=240)
        res[r] = (loss, g, same)
    for p in procs:
        p.join(timeout=60)
    for r, (loss, g, _) in res.items():
        assert g is not None, f"rank {r} failed: {loss}"
    shards, hg, ref = _case(W, n, d)
    eloss, egrads = _emulate(shards, compute)
    bound, _ = _bound(hg, ref, compute)
    for r in range(W):
        loss, g, same = res[r]
        assert same, f"rank {r}: overlap=True and overlap=False differ"
        assert loss == res[0][0]  # identical on all ranks
        assert abs(loss - eloss) <= 1e-6 * abs(eloss), (r, loss, eloss)  # (the all-reduce order may differ)
        assert torch.equal(torch.from_numpy(g), egrads[r].cpu()), f"rank {r}: gradient differs from the emulation's"
    e = _errors(res[0][0], _join([torch.from_numpy(res[r][1]) for r in range(W)]).cuda(), ref)
    print(f"XVDISTPROC {backend} W={W} n={n} d={d} compute={compute} loss/dh={e[0]:.3e}/{e[1]:.3e} "
          f"bound={bound[0]:.3e}/{bound[1]:.3e}")
    assert e[0] <= bound[0] and e[1] <= bound[1], (e, bound)


@pytest.mark.parametrize("W,n,d,compute", [(2, 150, 100, "fp16"), (3, 129, 160, "fp32")])
def test_multiprocess_gloo(gpu, W, n, d, compute):
    _run_and_check(W, n, d, compute, "gloo")


@pytest.mark.parametrize("W,n,d,compute", [(2, 150, 100, "fp16"), (8, 37, 40, "fp32")])
def test_multiprocess_rccl(gpu, W, n, d, compute):
    _run_and_check(W, n, d, compute, "nccl")


# ---- 5. repeatability and fall-back ------------------------------------------------------------------------
@pytest.mark.parametrize("W,n,d,compute", [(3, 129, 160, "fp16"), (2, 200, 100, "bf16")])
def test_two_runs_are_bitwise_equal(gpu, W, n, d, compute):
    shards, _, _ = _case(W, n, d)
    l0, g0 = _emulate(shards, compute)
    l1, g1 = _emulate(shards, compute)
    assert l0 == l1 and all(torch.equal(a, b) for a, b in zip(g0, g1))


@pytest.mark.parametrize("compute", ["fp32", "fp16", "fp8"])
def test_without_a_process_group_it_is_info_nce_loss(gpu, compute):
    from ntxent_amd.parallel import DistInfoNCELoss, dist_info_nce_loss

    (h,) = _shards(1, 200, 100)
    want = _one_gpu(h, compute)
    for fn in (lambda x: dist_info_nce_loss(x, T, compute=compute),
               lambda x: dist_info_nce_loss(x[:200], T, z2=x[200:], compute=compute),
               lambda x: DistInfoNCELoss(T, compute=compute)(x)):
        x = h.clone().requires_grad_(True)
        loss = fn(x)
        (g,) = torch.autograd.grad(loss, x, torch.tensor(GO, device=x.device))
        assert loss.item() == want[0] and torch.equal(g, want[1])


def test_does_not_disturb_ntxent(gpu):
    """An emulated step between ntxent_loss's forward and backward changes neither."""
    _, h = _inputs(1024, 256, torch.bfloat16, seed=9)
    shards = _shards(2, 200, 100)
    alone = _emulate(shards, "fp16")

    def run(between):
        x = h.clone().requires_grad_(True)
        loss = ntxent_amd.ntxent_loss(x, 0.1)
        got = _emulate(shards, "fp16") if between else None
        loss.backward()
        return loss.detach().clone(), x.grad.clone(), got

    l0, g0, _ = run(False)
    l1, g1, got = run(True)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    assert got[0] == alone[0] and all(torch.equal(a, b) for a, b in zip(got[1], alone[1]))
