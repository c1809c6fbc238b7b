"""Distributed cross-view InfoNCE (parallel/infonce.py) on the CPU: the gloo algorithm against the
fp64 oracle on the global batch in pair order, the fall-backs and refusals, the cross-view
cross-block probes of ops/reference.py boundary_probes, and the input conditions of the planted
inputs that tests/test_gpu_infonce_dist.py runs (dist_probe_case, shared with it).
"""
import functools
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ntxent_amd.ops import reference as R
from test_probes_cpu import TAU, decoys, two_views

PROBE_DIMS = {300: 100, 258: 160}  # rows per rank -> d (258: n = 129, two tiles per side, the second one row)
PROBE_SHAPES = [(W, rows) for W in (2, 3) for rows in (300, 258)]


@functools.lru_cache(maxsize=None)
def dist_probe_case(W, rows):
    """(planted fp64 input in global pair order, probes mapped into it, labels): two_views per rank,
    every probe planted at c = 0.55 and four same-view decoys at 0.9 (tests/test_probes_cpu.py
    probe_case, for W blocks of cross-view rows)."""
    dim = PROBE_DIMS[rows]
    probes, labels = R.boundary_probes(rows, 128, blocks=W, cross_view=True, return_labels=True)
    m = R.stacked_to_pair_order(W, rows).tolist()
    probes = [(m[i], m[j]) for i, j in probes]
    h = R.global_pair_order([two_views(rows, dim, seed=rows + dim + 101 * r) for r in range(W)])
    h = R.plant_pairs(h, probes, 0.55)
    return R.plant_pairs(h, decoys(W * rows, probes), 0.9), probes, labels


# ---- gloo ----------------------------------------------------------------------------------------
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n, dim, T, grad_out, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ntxent_amd.parallel import DistInfoNCELoss, dist_info_nce_loss

        g = torch.Generator().manual_seed(1000 + rank)
        h = torch.randn(2 * n, dim, generator=g, dtype=torch.float64).requires_grad_(True)
        loss = dist_info_nce_loss(h, T)  # CPU rows: cpu_dist_info_nce_loss
        loss.backward(torch.tensor(grad_out, dtype=torch.float64))
        via_module = DistInfoNCELoss(T)(h.detach()[:n], h.detach()[n:])
        q.put((rank, loss.detach().numpy().copy(), h.detach().numpy().copy(), h.grad.detach().numpy().copy(),
               via_module.numpy().copy()))
    finally:
        dist.destroy_process_group()


def _run(world, n, dim, T, grad_out):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, dim, T, grad_out, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return [tuple(torch.from_numpy(x) for x in o[1:]) for o in sorted(out, key=lambda x: x[0])]


@pytest.mark.parametrize("world,n,dim", [(2, 4, 8), (2, 5, 17), (3, 3, 6)])
def test_gloo_matches_oracle(world, n, dim):
    T, go = 0.1, 0.7
    res = _run(world, n, dim, T, go)
    hg = R.global_pair_order([r[1] for r in res]).requires_grad_(True)
    l_ref = R.info_nce_loss(hg, T)
    (g_ref,) = torch.autograd.grad(l_ref, hg, torch.tensor(go, dtype=hg.dtype))
    N = world * n
    for r, (loss, _, grad, via_module) in enumerate(res):
        torch.testing.assert_close(loss, l_ref.detach(), rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(via_module, loss, rtol=0, atol=0)
        torch.testing.assert_close(grad[:n], g_ref[r * n:(r + 1) * n], rtol=1e-9, atol=1e-12)
        torch.testing.assert_close(grad[n:], g_ref[N + r * n:N + (r + 1) * n], rtol=1e-9, atol=1e-12)


# ---- no process group, refusals --------------------------------------------------------------------
def test_without_a_process_group_it_is_the_reference():
    from ntxent_amd.parallel import DistInfoNCELoss, cpu_dist_info_nce_loss, dist_info_nce_loss

    h = two_views(40, 12, seed=3)
    want = R.info_nce_loss(h, 0.2)
    (gw,) = torch.autograd.grad(R.info_nce_loss(x := h.clone().requires_grad_(True), 0.2), x)
    assert torch.equal(dist_info_nce_loss(h, 0.2), want)
    assert torch.equal(dist_info_nce_loss(h[:20], 0.2, z2=h[20:]), want)
    assert torch.equal(DistInfoNCELoss(0.2)(h[:20], h[20:]), want)
    x = h.clone().requires_grad_(True)
    loss = cpu_dist_info_nce_loss(x, 0.2)  # the gloo algorithm with one rank
    torch.testing.assert_close(loss, want, rtol=1e-12, atol=0)
    torch.testing.assert_close(torch.autograd.grad(loss, x)[0], gw, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("make", [lambda: torch.tensor(0.1, requires_grad=True),
                                  lambda: torch.tensor(-2.0, requires_grad=True).exp()])
def test_a_temperature_that_requires_grad_is_refused(make):
    from ntxent_amd.parallel import DistInfoNCELoss, cpu_dist_info_nce_loss, dist_info_nce_loss

    h = two_views(16, 8, seed=1).float()
    for call in (lambda t: dist_info_nce_loss(h, t), lambda t: cpu_dist_info_nce_loss(h, t),
                 lambda t: DistInfoNCELoss(t)(h)):
        with pytest.raises(NotImplementedError, match="requires grad"):
            call(make())
    assert torch.isfinite(dist_info_nce_loss(h, torch.tensor(0.1)))  # a detached tensor is a float


# ---- the cross-view cross-block probes --------------------------------------------------------------
@pytest.mark.parametrize("W,rows", PROBE_SHAPES)
def test_cross_block_probes(W, rows):
    probes, labels = R.boundary_probes(rows, 128, blocks=W, cross_view=True, return_labels=True)
    assert probes == R.boundary_probes(rows, 128, blocks=W, cross_view=True)
    n, total = rows // 2, rows * W

    def pos(k):
        return k // rows * rows + (k % rows + n) % rows

    used = [k for p in probes for k in p]
    assert all(0 <= k < total for k in used)
    assert len(set(used)) == len(used)  # every row in at most one probe
    assert not {i for i, _ in probes} & {j for _, j in probes}  # no i is another probe's j
    assert not {pos(k) for k in used} & set(used)  # no probe row is the positive of a probe row
    assert all(j != i and j != pos(i) for i, j in probes)
    assert all((i % rows >= n) != (j % rows >= n) for i, j in probes)  # every probe is cross-view
    cross = [(p, l) for p, l in zip(probes, labels) if "cross-block" in l]
    inside = [p for p, l in zip(probes, labels) if "cross-block" not in l]
    assert all(i // rows == j // rows for i, j in inside)
    # the list of one block is unchanged, and every block carries it
    one = R.boundary_probes(rows, 128, cross_view=True)
    assert not any("cross-block" in l for l in R.boundary_probes(rows, 128, cross_view=True, return_labels=True)[1])
    for b in range(W):
        assert [(i - b * rows, j - b * rows) for i, j in inside if i // rows == b] == one
    local = lambda k: k % rows % n  # index within the view
    for a in range(W if W > 2 else 1):
        b = (a + 1) % W
        for src, dst in ((a, b), (b, a)):  # both directions
            mine = {l[1]: p for p, l in cross if p[0] // rows == src and p[1] // rows == dst}
            assert set(mine) == {"would-be", "pos+1", "pos-1", "last-col", "first-col"}, (src, dst, mine)
            assert local(mine["would-be"][1]) == local(mine["would-be"][0])
            assert local(mine["pos+1"][1]) == local(mine["pos+1"][0]) + 1
            assert local(mine["pos-1"][1]) == local(mine["pos-1"][0]) - 1
            assert n - 16 <= local(mine["last-col"][1]) <= n - 1 and local(mine["first-col"][1]) <= 15  # the edge 16 x 16 fragment
            assert {i % rows >= n for i, _ in mine.values()} == {True, False}  # rows of both sides
    assert len(cross) == 10 * (W if W > 2 else 1)


def test_the_existing_lists_do_not_change():
    """The lists of every combination that existed before the cross-view cross-block category
    (blocks = 1, and same-view blocks), by the sha256 of their repr, recorded before it was added."""
    import hashlib

    want = {(400, 128, 1, True): "906eedb6e919fe8a", (768, 128, 1, True): "8728ce149cd50507",
            (300, 128, 1, True): "3ace484b3ec70008", (258, 128, 1, True): "5888b40691d59213",
            (300, 256, 2, False): "999ff79e721b057e", (600, 256, 3, False): "0f397001e1b08077",
            (600, 64, 1, False): "b43d85640c298643"}
    for (rows, tile, blocks, xv), digest in want.items():
        probes = R.boundary_probes(rows, tile, blocks=blocks, cross_view=xv)
        assert hashlib.sha256(repr(probes).encode()).hexdigest()[:16] == digest, (rows, tile, blocks, xv)


@pytest.mark.parametrize("W,rows", PROBE_SHAPES)
def test_planting_and_input_conditions(W, rows):
    h, probes, _ = dist_probe_case(W, rows)
    assert h.dtype == torch.float64 and h.shape == (W * rows, PROBE_DIMS[rows])
    z, _ = R.normalize(h)
    ii, jj = torch.tensor(probes).t()
    assert ((z[ii] * z[jj]).sum(1) - 0.55).abs().max().item() <= 1e-12
    sig, p_ij = R.probe_signatures(h, TAU, probes, cross_view=True)
    print(f"PROBECPU xview-dist W={W} rows={rows} probes={len(probes)} P_ij={p_ij.min():.2f}..{p_ij.max():.2f} "
          f"sig_min={sig.min():.3f}")
    assert sig.min().item() >= 0.2
    assert 0.15 <= p_ij.min().item() and p_ij.max().item() <= 0.85
