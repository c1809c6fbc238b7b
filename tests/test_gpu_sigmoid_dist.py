"""Distributed pairwise sigmoid loss (parallel/sigmoid.py, the xview_sigmoid_* kernels of
csrc/kernels/xview_kernels.hip over rank slots) on an MI355X: W virtual ranks through the emulation,
and W real processes on the one GPU over gloo and RCCL, against the fp64 oracle
``reference.sigmoid_loss`` on the global batch in pair order.

Bounds come from the project, not from the code under test. Per quantity (loss relative with floor 1,
dh max-abs over the global max|g|, dtau relative, dbias relative to the oracle's (1/N) sum |G|):
2 x max(test_gpu_sigmoid.TABLE[compute] (dbias: dtau's value), the error the one-GPU sigmoid_loss
shows on the same global batch against the same oracle, same compute, tau, bias, same run). The exact
cases take test_gpu_sigmoid._fp32_bound's rule on the global batch in every compute dtype. Every
gradient is taken at grad_out = 0.7.

Largest errors measured on MI355X over the parity shapes below (loss / dh / dtau / dbias): fp32 6.8e-8 /
2.6e-6 / 7.4e-8 / 1.1e-7, fp16 1.9e-7 / 1.0e-3 / 2.1e-5 / 1.5e-7, bf16 6.8e-7 / 4.9e-3 / 3.1e-5 / 8.5e-7; the
one-GPU sigmoid_loss on the same global batches in the same run: fp32 the same four, fp16 1.9e-7 / 1.0e-3 /
2.1e-5 / 1.3e-7, bf16 the same four (profiles/sigmoid_dist/parity.log). The probes' smallest single-pair
term is 0.233 of the global max|g| (W = 3, 258 rows per rank).
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
from ntxent_amd.parallel.emulate import emulated_sigmoid_forward_backward
from test_gpu_sigmoid import PAIRS, TABLE, _errors, _fmt, _fp32_bound, _inputs, _oracle, _run, _softplus, _t
from test_infonce_dist_cpu import PROBE_SHAPES, dist_probe_case

pytestmark = pytest.mark.gpu

GO = 0.7


def _shards(W, n, d):
    return [_inputs(2 * n, d, torch.float32, seed=n + d + 101 * r) for r in range(W)]


def _split(hg, W):
    """The rank shards [a_r; b_r] of a global batch in pair order."""
    N = hg.shape[0] // 2
    n = N // W
    return [torch.cat([hg[r * n:(r + 1) * n], hg[N + r * n:N + (r + 1) * n]], 0).contiguous() for r in range(W)]


def _join(grads):
    n = grads[0].shape[0] // 2
    return torch.cat([g[:n] for g in grads] + [g[n:] for g in grads], 0)


def _oracle_go(hg, T, bias):
    """test_gpu_sigmoid._oracle's tuple with every gradient (and the dbias scale) times GO."""
    loss, gh, gt, gb, gabs = _oracle(hg, T, bias)
    return loss, GO * gh, GO * gt, GO * gb, GO * gabs


def _emulate(shards, T, bias, compute, go=GO, **kw):
    loss, grads, dtau, dbias = emulated_sigmoid_forward_backward(shards, T, bias, compute=compute, grad_out=go, **kw)
    torch.cuda.synchronize()
    return loss, grads, dtau, dbias


def _bound(hg, T, bias, compute, ref):
    """Group 1's bound on this global batch, and the one-GPU errors it was taken from."""
    e_old = _errors(_run(hg, _t(T), _t(bias), compute, scale=GO), ref)
    tab = TABLE[compute] + (TABLE[compute][2],)
    return tuple(2.0 * max(t, e) for t, e in zip(tab, e_old)), e_old


@functools.lru_cache(maxsize=None)
def _case(W, n, d, T, bias):
    shards = _shards(W, n, d)
    hg = R.global_pair_order(shards)
    return shards, hg, _oracle_go(hg, T, bias)


# ---- 1. emulated parity with the fp64 oracle on the global batch ----------------------------------------
CASES = [(2, 37, 40, "fp32"), (3, 129, 160, "fp32"), (3, 129, 160, "fp16"), (2, 200, 100, "bf16"),
         (4, 128, 64, "fp32"), (8, 37, 40, "fp16"),
         # world 1: the stage ops as the one-GPU op rides on them
         (1, 129, 160, "fp16"), (1, 37, 40, "fp32")]


@pytest.mark.parametrize("T,bias", PAIRS)
@pytest.mark.parametrize("W,n,d,compute", CASES)
def test_emulated_parity_with_the_oracle(gpu, W, n, d, compute, T, bias):
    """At (0.5, 0) every pair carries about 0.69 / N^2 of the loss, above every compute's bound: one
    dropped or doubly counted element fails. At (0.1, -10) the positives carry the loss: a positive
    taken from the wrong slot, or missed, fails."""
    shards, hg, ref = _case(W, n, d, T, bias)
    loss, grads, dtau, dbias = _emulate(shards, T, bias, compute)
    e_new = _errors((loss, _join(grads), dtau, dbias), ref)
    bound, e_old = _bound(hg, T, bias, compute, ref)
    print(f"SIGDIST W={W} n={n} d={d} compute={compute} tau={T} bias={bias} dist loss/dh/dtau/dbias={_fmt(e_new)} "
          f"one-GPU={_fmt(e_old)} bound={_fmt(bound)}")
    assert all(math.isfinite(e) for e in e_new)
    assert all(e <= b for e, b in zip(e_new, bound)), (e_new, bound)


# ---- 2. exact cases -----------------------------------------------------------------------------------
@pytest.mark.parametrize("T,bias", PAIRS)
@pytest.mark.parametrize("compute", ["fp32", "fp16", "bf16"])
def test_identical_rows(gpu, compute, T, bias):
    """Every cosine is 1 (the exactly representable row of test_gpu_sigmoid.test_identical_rows):
    loss = softplus(-x) + (N - 1) softplus(x), x = 1 / tau + bias; a counted pad column or slot gap, or
    a positive per slot instead of per pair, gives another number."""
    W, n = 3, 37
    N = W * n
    row = torch.zeros(40)
    row[:16] = 2.0 * torch.tensor([1, -1, 1, 1, -1, 1, -1, -1, 1, 1, -1, 1, 1, -1, -1, 1])
    hg = row.repeat(2 * N, 1).cuda()
    loss, grads, _, _ = _emulate(_split(hg, W), T, bias, compute)
    x = 1.0 / T + bias
    want = _softplus(-x) + (N - 1) * _softplus(x)
    bound = _fp32_bound(hg, T, bias)
    le = abs(loss.item() - want) / max(1.0, want)
    print(f"SIGDISTEXACT identical W={W} n={n} compute={compute} tau={T} bias={bias} loss_err={le:.3e} bound={bound[0]:.3e}")
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
    loss, grads, _, _ = _emulate(_split(hg, W), T, bias, compute)
    want = _softplus(-(1.0 / T + bias)) + (N - 1) * _softplus(bias)
    gref = GO * _oracle(hg, T, bias)[1]
    bound = _fp32_bound(hg, T, bias)
    le = abs(loss.item() - want) / max(1.0, want)
    ge = (_join(grads).double() - gref).abs().max().item() / gref.abs().max().item()
    print(f"SIGDISTEXACT orthogonal W={W} n={n} compute={compute} tau={T} bias={bias} loss_err={le:.3e} "
          f"bound={bound[0]:.3e} dh_err={ge:.3e} bound={bound[1]:.3e}")
    assert le <= bound[0], (loss.item(), want)
    assert ge <= bound[1]


# ---- 3. planted-pair probes -----------------------------------------------------------------------------
PROBE_T, PROBE_BIAS = 0.1, -5.0


def _pair_terms(x, g, probes, T, bias):
    """[k, 2]: for probe (i, j), a cross-view pair that is no positive, the size of that single pair's
    term in row i's and in row j's gradient, max| inv_a sigmoid(x_ab) / (N tau) (z_b - cos z_a) |, over
    the global max|g| (fp64)."""
    z, inv = R.normalize(x)
    N = x.shape[0] // 2
    ii, jj = torch.tensor(probes, device=x.device).t()
    cos = (z[ii] * z[jj]).sum(1, keepdim=True)
    G = torch.sigmoid(cos / T + bias) / (N * T)
    ti = (inv[ii].unsqueeze(1) * G * (z[jj] - cos * z[ii])).abs().amax(1)
    tj = (inv[jj].unsqueeze(1) * G * (z[ii] - cos * z[jj])).abs().amax(1)
    return torch.stack([ti, tj], 1) / g.abs().max()


@functools.lru_cache(maxsize=2)
def _probe_oracle(W, rows):
    h64, probes, labels = dist_probe_case(W, rows)
    hg = h64.float().cuda()
    ref = _oracle_go(hg, PROBE_T, PROBE_BIAS)
    sig = _pair_terms(hg.double(), ref[1] / GO, probes, PROBE_T, PROBE_BIAS)
    return hg, ref, sig.min().item(), probes, labels


@pytest.mark.parametrize("compute", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("W,rows", PROBE_SHAPES)
def test_planted_pair_probes(gpu, W, rows, compute):
    """Planted cross-view pairs (cos 0.55) in every rank's own block and across ranks (the other rank's
    would-be positive, its neighbours, the last and first valid columns of a slot), at tau = 0.1, bias =
    -5: each is one pair's term of at least sig_min of two rows' gradients, relative to the global
    max|g| (0.233 measured on the CPU over the four shapes)."""
    hg, ref, sig_min, probes, labels = _probe_oracle(W, rows)
    loss, grads, dtau, dbias = _emulate(_split(hg, W), PROBE_T, PROBE_BIAS, compute)
    g = _join(grads)
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    bound, _ = _bound(hg, PROBE_T, PROBE_BIAS, compute, ref)
    idx = torch.tensor(probes, device=g.device)
    rerr = (g[idx].double() - ref[1][idx]).abs().amax(2) / ref[1].abs().max()
    e_new = _errors((loss, g, dtau, dbias), ref)
    k = rerr.amax(1).argmax().item()
    print(f"PROBE sigmoid-dist W={W} rows={rows} compute={compute} probes={len(probes)} sig_min={sig_min:.3f} "
          f"row_err_max={rerr.max().item():.3e} at={probes[k]}{'/'.join(labels[k])} cap={sig_min / 4:.3e} "
          f"loss/dh/dtau/dbias={_fmt(e_new)} bound={_fmt(bound)}")
    assert sig_min >= 0.2, sig_min
    assert bound[1] <= sig_min / 4, (bound[1], sig_min)
    bad = [(probes[i], labels[i], [f"{e:.2e}" for e in rerr[i].tolist()]) for i in range(len(probes))
           if rerr[i].max().item() > bound[1]]
    assert not bad, f"probe rows over the dh bound {bound[1]:.2e}: {bad}"
    assert e_new[0] <= bound[0] and e_new[2] <= bound[2] and e_new[3] <= bound[3], (e_new, bound)


# ---- 4. scalar gradients --------------------------------------------------------------------------------
@pytest.mark.parametrize("W,n,d,compute", [(3, 129, 160, "fp16"), (2, 37, 40, "fp32")])
def test_dh_does_not_depend_on_the_scalar_gradients(gpu, W, n, d, compute):
    """The rank-local backward with neither scalar gradient (no shares: nothing to reduce), with one
    of them and with both: dh and the loss are bitwise the same, and each scalar is the same number."""
    shards, _, _ = _case(W, n, d, 0.1, -10.0)
    both = _emulate(shards, 0.1, -10.0, compute)
    for want_tau, want_bias in [(False, False), (True, False), (False, True)]:
        got = _emulate(shards, 0.1, -10.0, compute, want_tau=want_tau, want_bias=want_bias)
        assert torch.equal(got[0], both[0]) and all(torch.equal(a, b) for a, b in zip(got[1], both[1]))
        assert (got[2] is None) == (not want_tau) and (got[3] is None) == (not want_bias)
        assert got[2] is None or torch.equal(got[2], both[2])
        assert got[3] is None or torch.equal(got[3], both[3])


def test_grad_out_scaling(gpu):
    """test_gpu_sigmoid.test_grad_out_scaling's 2e-7 (three fp32 roundings), for all three gradients."""
    shards, _, _ = _case(3, 129, 160, 0.1, -10.0)
    _, g1, t1, b1 = _emulate(shards, 0.1, -10.0, "fp32", go=1.0)
    _, g35, t35, b35 = _emulate(shards, 0.1, -10.0, "fp32", go=3.5)
    g1, g35 = _join(g1), _join(g35)
    assert (g35 - 3.5 * g1).abs().max().item() <= 2e-7 * (3.5 * g1).abs().max().item()
    assert abs(t35.item() - 3.5 * t1.item()) <= 2e-7 * abs(3.5 * t1.item())
    assert abs(b35.item() - 3.5 * b1.item()) <= 2e-7 * abs(3.5 * b1.item())


# ---- 5. real processes on the one GPU ---------------------------------------------------------------------
PROC_T, PROC_BIAS = 0.1, -10.0


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
        from ntxent_amd.parallel import dist_sigmoid_loss

        go = torch.tensor(GO, device="cuda")

        def step(tau, bias, overlap=True):
            h = _shards(W, n, d)[rank].requires_grad_(True)
            loss = dist_sigmoid_loss(h, tau, bias, compute=compute, overlap=overlap)
            leaves = [v for v in (tau, bias) if isinstance(v, torch.Tensor)]
            grads = torch.autograd.grad(loss, [h] + leaves, go)
            torch.cuda.synchronize()
            return loss, grads

        out = [step(_t(PROC_T), _t(PROC_BIAS), overlap) for overlap in (True, False)]
        same = all(torch.equal(a, b) for a, b in zip((out[0][0],) + out[0][1], (out[1][0],) + out[1][1]))
        # float arguments (a backward that does not communicate) and one tensor alone: the same loss and dh
        for tau, bias in ((PROC_T, PROC_BIAS), (_t(PROC_T), PROC_BIAS), (PROC_T, _t(PROC_BIAS))):
            loss, grads = step(tau, bias)
            same = same and torch.equal(loss, out[0][0]) and torch.equal(grads[0], out[0][1][0])
            if len(grads) == 2:
                same = same and torch.equal(grads[1], out[0][1][1 if isinstance(tau, torch.Tensor) else 2])
        loss, (g, dtau, dbias) = out[0]
        q.put((rank, loss.item(), g.cpu().numpy(), dtau.item(), dbias.item(), same))  # by value
    except Exception as e:  # surface the failure in the parent
        q.put((rank, repr(e), None, None, None, False))
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
    eloss, egrads, etau, ebias = _emulate(shards, PROC_T, PROC_BIAS, compute)
    bound, _ = _bound(hg, PROC_T, PROC_BIAS, compute, ref)
    for r in range(W):
        loss, g, dtau, dbias, same = res[r]
        assert same, f"rank {r}: overlap, float or single-tensor arguments change the loss, dh or a scalar gradient"
        assert (loss, dtau, dbias) == tuple(res[0][i] for i in (0, 2, 3))  # identical on all ranks
        for got, emu in ((loss, eloss), (dtau, etau), (dbias, ebias)):  # (the all-reduce order may differ)
            assert abs(got - emu.item()) <= 1e-6 * abs(emu.item()), (r, got, emu.item())
        assert torch.equal(torch.from_numpy(g), egrads[r].cpu()), f"rank {r}: gradient differs from the emulation's"
    dev = hg.device
    e = _errors((torch.tensor(res[0][0]), _join([torch.from_numpy(res[r][1]) for r in range(W)]).to(dev),
                 torch.tensor(res[0][2]), torch.tensor(res[0][3])), ref)
    print(f"SIGDISTPROC {backend} W={W} n={n} d={d} compute={compute} loss/dh/dtau/dbias={_fmt(e)} bound={_fmt(bound)}")
    assert all(x <= b for x, b in zip(e, bound)), (e, bound)


def test_multiprocess_gloo(gpu):
    _run_and_check(2, 150, 100, "fp16", "gloo")


def test_multiprocess_rccl(gpu):
    _run_and_check(3, 129, 160, "fp32", "nccl")


# ---- 6. repeatability and fall-back ------------------------------------------------------------------------
@pytest.mark.parametrize("W,n,d,compute", [(3, 129, 160, "fp16"), (2, 200, 100, "bf16")])
def test_two_runs_are_bitwise_equal(gpu, W, n, d, compute):
    shards, _, _ = _case(W, n, d, 0.1, -10.0)
    a = _emulate(shards, 0.1, -10.0, compute)
    b = _emulate(shards, 0.1, -10.0, compute)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("compute", ["fp32", "fp16", "fp8"])
def test_without_a_process_group_it_is_sigmoid_loss(gpu, compute):
    from ntxent_amd.parallel import DistSigmoidLoss, dist_sigmoid_loss

    (h,) = _shards(1, 200, 100)
    want = _run(h, _t(0.1), _t(-10.0), compute, scale=GO)
    for fn in (lambda x: dist_sigmoid_loss(x, 0.1, -10.0, compute=compute),
               lambda x: dist_sigmoid_loss(x[:200], 0.1, -10.0, z2=x[200:], compute=compute),
               lambda x: DistSigmoidLoss(0.1, -10.0, compute=compute)(x)):
        x = h.clone().requires_grad_(True)
        loss = fn(x)
        (g,) = torch.autograd.grad(loss, x, torch.tensor(GO, device=x.device))
        assert torch.equal(loss.detach(), want[0]) and torch.equal(g, want[1])
    x, tau, bias = h.clone().requires_grad_(True), _t(0.1), _t(-10.0)
    (GO * dist_sigmoid_loss(x, tau, bias, compute=compute)).backward()
    assert torch.equal(tau.grad, want[2]) and torch.equal(bias.grad, want[3])


def test_does_not_disturb_sigmoid_loss(gpu):
    """An emulated step between sigmoid_loss's forward and backward changes neither."""
    h = _inputs(1024, 256, torch.bfloat16, seed=9)
    shards = _shards(2, 200, 100)
    alone = _emulate(shards, 0.1, -10.0, "fp16")

    def run(between):
        x = h.clone().requires_grad_(True)
        loss = ntxent_amd.sigmoid_loss(x, 0.1, -10.0)
        got = _emulate(shards, 0.1, -10.0, "fp16") if between else None
        loss.backward()
        return loss.detach().clone(), x.grad.clone(), got

    l0, g0, _ = run(False)
    l1, g1, got = run(True)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    assert torch.equal(got[0], alone[0]) and all(torch.equal(a, b) for a, b in zip(got[1], alone[1]))
    assert torch.equal(got[2], alone[2]) and torch.equal(got[3], alone[3])
