"""Distributed pairwise sigmoid loss (parallel/sigmoid.py) on the CPU: the gloo algorithm against the
fp64 oracle ``reference.sigmoid_loss`` on the global batch in pair order, with both scalar gradients
(all-reduced, equal on every rank), the fall-backs, and the refusal of multi-element arguments. The
tolerances are those of tests/test_infonce_dist_cpu.py.
"""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ntxent_amd.ops import reference as R
from ntxent_amd.parallel import DistSigmoidLoss, cpu_dist_sigmoid_loss, dist_sigmoid_loss
from test_probes_cpu import two_views

GO = 0.7
PAIRS = [(0.1, -10.0), (0.5, 0.0)]  # (tau, bias)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _leaf(v):
    return torch.tensor(v, dtype=torch.float64, requires_grad=True)


def _worker(rank, world, port, n, dim, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = torch.Generator().manual_seed(1000 + rank)
        h = torch.randn(2 * n, dim, generator=g, dtype=torch.float64)
        out = [h.numpy().copy()]
        for T, bias in PAIRS:
            x, tau, b = h.clone().requires_grad_(True), _leaf(T), _leaf(bias)
            loss = dist_sigmoid_loss(x, tau, b)  # CPU rows: cpu_dist_sigmoid_loss
            loss.backward(torch.tensor(GO, dtype=torch.float64))
            m = DistSigmoidLoss(T, bias)(h[:n], h[n:])
            out += [loss.detach().numpy().copy(), x.grad.numpy().copy(), tau.grad.numpy().copy(), b.grad.numpy().copy(),
                    m.numpy().copy()]
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def _run(world, n, dim):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, dim, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return [[torch.from_numpy(x) for x in o[1]] for o in sorted(out, key=lambda x: x[0])]


@pytest.mark.parametrize("world,n,dim", [(2, 4, 8), (2, 5, 17), (3, 3, 6)])
def test_gloo_matches_oracle(world, n, dim):
    res = _run(world, n, dim)
    N = world * n
    for k, (T, bias) in enumerate(PAIRS):
        hg = R.global_pair_order([r[0] for r in res]).requires_grad_(True)
        tau, b = _leaf(T), _leaf(bias)
        l_ref = R.sigmoid_loss(hg, tau, b)
        g_ref, t_ref, b_ref = torch.autograd.grad(l_ref, (hg, tau, b), torch.tensor(GO, dtype=hg.dtype))
        for r in range(world):
            loss, grad, dtau, dbias, via_module = res[r][1 + 5 * k:6 + 5 * k]
            torch.testing.assert_close(loss, l_ref.detach(), rtol=1e-10, atol=1e-12)
            torch.testing.assert_close(via_module, loss, rtol=0, atol=0)
            torch.testing.assert_close(grad[:n], g_ref[r * n:(r + 1) * n], rtol=1e-9, atol=1e-12)
            torch.testing.assert_close(grad[n:], g_ref[N + r * n:N + (r + 1) * n], rtol=1e-9, atol=1e-12)
            torch.testing.assert_close(dtau, t_ref, rtol=1e-9, atol=1e-12)
            torch.testing.assert_close(dbias, b_ref, rtol=1e-9, atol=1e-12)
            # identical on every rank: the all-reduced numbers
            for a, c in zip((loss, dtau, dbias), (res[0][1 + 5 * k], res[0][3 + 5 * k], res[0][4 + 5 * k])):
                assert torch.equal(a, c)


def test_without_a_process_group_it_is_sigmoid_loss():
    import ntxent_amd

    h = two_views(40, 12, seed=3)
    want = ntxent_amd.sigmoid_loss(h, 0.2, -3.0)
    assert torch.equal(dist_sigmoid_loss(h, 0.2, -3.0), want)
    assert torch.equal(dist_sigmoid_loss(h[:20], 0.2, -3.0, z2=h[20:]), want)
    assert torch.equal(DistSigmoidLoss(0.2, -3.0)(h[:20], h[20:]), want)
    x, tau, b = h.clone().requires_grad_(True), _leaf(0.2), _leaf(-3.0)
    gw = torch.autograd.grad(R.sigmoid_loss(x, tau, b), (x, tau, b))
    loss = cpu_dist_sigmoid_loss(x, tau, b)  # the gloo algorithm with one rank
    torch.testing.assert_close(loss, R.sigmoid_loss(h, 0.2, -3.0), rtol=1e-12, atol=0)
    for got, ref in zip(torch.autograd.grad(loss, (x, tau, b)), gw):
        torch.testing.assert_close(got, ref, rtol=1e-9, atol=1e-12)


def test_learnable_module_owns_both_parameters():
    m = DistSigmoidLoss(0.1, -10.0, learnable_temperature=True, learnable_bias=True)
    assert {n for n, _ in m.named_parameters()} == {"log_temperature", "bias"}
    m(two_views(16, 8, seed=2).float()).backward()
    assert m.log_temperature.grad is not None and m.bias.grad is not None


@pytest.mark.parametrize("which", ["temperature", "bias"])
def test_a_multi_element_argument_is_refused(which):
    h = two_views(16, 8, seed=1).float()
    kw = {which: torch.tensor([0.1, 0.2])}
    for call in (dist_sigmoid_loss, cpu_dist_sigmoid_loss):
        with pytest.raises(ValueError, match=which):
            call(h, **kw)
