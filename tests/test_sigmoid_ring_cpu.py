"""``exchange="ring"`` of the distributed pairwise sigmoid loss (parallel/sigmoid.py) on the CPU: the gloo
send / recv ring against the fp64 oracle ``reference.sigmoid_loss`` on the global batch in pair order,
with both scalar gradients, the module's parameters, the fall-back and the refusal of an unknown
exchange. The tolerances are those of tests/test_sigmoid_dist_cpu.py; the module's parameters are
float32, so their gradients are compared at 1e-6 relative (one fp32 rounding is 6e-8) against the
oracle at the parameters' own float32 values.
"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ntxent_amd.ops import reference as R
from ntxent_amd.parallel import DistSigmoidLoss, cpu_dist_sigmoid_loss, dist_sigmoid_loss
from test_probes_cpu import two_views
from test_sigmoid_dist_cpu import GO, PAIRS, _free_port, _leaf


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
            loss = dist_sigmoid_loss(x, tau, b, exchange="ring")  # CPU rows: the gloo ring
            loss.backward(torch.tensor(GO, dtype=torch.float64))
            gather = dist_sigmoid_loss(h, T, bias)
            m = DistSigmoidLoss(T, bias, exchange="ring", learnable_temperature=True, learnable_bias=True)
            before = (m.current_temperature().item(), m.bias.item())  # the float32 values the step runs at
            logt = m.log_temperature.item()
            opt = torch.optim.SGD(m.parameters(), lr=0.5)
            m(h[:n], h[n:]).backward()
            grads = torch.stack([m.log_temperature.grad.double(), m.bias.grad.double()])
            opt.step()
            moved = torch.tensor([float(m.log_temperature.item() != logt), float(m.bias.item() != before[1])])
            out += [loss.detach().numpy().copy(), x.grad.numpy().copy(), tau.grad.numpy().copy(), b.grad.numpy().copy(),
                    gather.numpy().copy(), grads.numpy().copy(), moved.numpy().copy(), torch.tensor(before).numpy().copy()]
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
def test_gloo_ring_matches_oracle(world, n, dim):
    res = _run(world, n, dim)
    N = world * n
    K = 8
    for k, (T, bias) in enumerate(PAIRS):
        hg = R.global_pair_order([r[0] for r in res]).requires_grad_(True)
        tau, b = _leaf(T), _leaf(bias)
        l_ref = R.sigmoid_loss(hg, tau, b)
        g_ref, t_ref, b_ref = torch.autograd.grad(l_ref, (hg, tau, b), torch.tensor(GO, dtype=hg.dtype))
        for r in range(world):
            loss, grad, dtau, dbias, gather, mgrads, moved, before = res[r][1 + K * k:1 + K * (k + 1)]
            torch.testing.assert_close(loss, l_ref.detach(), rtol=1e-10, atol=1e-12)
            torch.testing.assert_close(gather, l_ref.detach(), rtol=1e-10, atol=1e-12)  # the gather path beside it
            torch.testing.assert_close(grad[:n], g_ref[r * n:(r + 1) * n], rtol=1e-9, atol=1e-12)
            torch.testing.assert_close(grad[n:], g_ref[N + r * n:N + (r + 1) * n], rtol=1e-9, atol=1e-12)
            torch.testing.assert_close(dtau, t_ref, rtol=1e-9, atol=1e-12)
            torch.testing.assert_close(dbias, b_ref, rtol=1e-9, atol=1e-12)
            # identical on every rank: the all-reduced numbers
            for a, c in zip((loss, dtau, dbias), (res[0][1 + K * k], res[0][3 + K * k], res[0][4 + K * k])):
                assert torch.equal(a, c)
            # the module's parameters (float32): the oracle's gradients at their own values, d/dlog tau = tau d/dtau
            tm, bm = _leaf(before[0].item()), _leaf(before[1].item())
            tg, bg = torch.autograd.grad(R.sigmoid_loss(hg.detach(), tm, bm), (tm, bm))
            torch.testing.assert_close(mgrads, torch.stack([tg * tm.detach(), bg]), rtol=1e-6, atol=1e-12)
            assert moved.tolist() == [1.0, 1.0]  # an SGD step moves both: they train


def test_an_unknown_exchange_is_refused():
    h = two_views(16, 8, seed=1).float()
    for call in (dist_sigmoid_loss, cpu_dist_sigmoid_loss):
        with pytest.raises(ValueError, match="exchange"):
            call(h, 0.1, -10.0, exchange="bogus")
    with pytest.raises(ValueError, match="exchange"):
        DistSigmoidLoss(0.1, -10.0, exchange="bogus")


def test_one_rank_falls_back_to_sigmoid_loss():
    import ntxent_amd

    h = two_views(40, 12, seed=3)
    want = ntxent_amd.sigmoid_loss(h, 0.2, -3.0)
    assert torch.equal(dist_sigmoid_loss(h, 0.2, -3.0, exchange="ring"), want)
    assert torch.equal(dist_sigmoid_loss(h[:20], 0.2, -3.0, z2=h[20:], exchange="ring"), want)
    assert torch.equal(DistSigmoidLoss(0.2, -3.0, exchange="ring")(h[:20], h[20:]), want)
    x, tau, b = h.clone().requires_grad_(True), _leaf(0.2), _leaf(-3.0)
    gw = torch.autograd.grad(R.sigmoid_loss(x, tau, b), (x, tau, b))
    loss = cpu_dist_sigmoid_loss(x, tau, b, exchange="ring")  # the ring algorithm with one rank: the own block alone
    torch.testing.assert_close(loss, R.sigmoid_loss(h, 0.2, -3.0), rtol=1e-12, atol=0)
    for got, ref in zip(torch.autograd.grad(loss, (x, tau, b)), gw):
        torch.testing.assert_close(got, ref, rtol=1e-9, atol=1e-12)


def test_ring_module_trains_both_parameters():
    m = DistSigmoidLoss(0.1, -10.0, exchange="ring", learnable_temperature=True, learnable_bias=True)
    assert {n for n, _ in m.named_parameters()} == {"log_temperature", "bias"}
    assert "exchange=ring" in repr(m)
    m(two_views(16, 8, seed=2).float()).backward()
    assert m.log_temperature.grad is not None and m.bias.grad is not None
