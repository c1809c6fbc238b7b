"""The fused InfoNCE backward (``backward="fused"``: no stored coefficient block) against the fp64
oracle, under the bound of tests/test_gpu_infonce.py: 2 x max(TABLE[compute], the error ntxent_loss
shows against its own oracle on the same input in the same run) for (loss, dh, dtau)."""
import functools

import pytest
import torch

import ntxent_amd
from ntxent_amd.ops import reference as R
from ntxent_amd.parallel.emulate import emulated_xview_forward_backward

pytestmark = pytest.mark.gpu

# tests/test_gpu_infonce.py's: (loss rtol, dh err / max|g|, dtau rtol)
TABLE = {"fp32": (2e-9, 6e-6, 4.5e-7), "fp16": (1.2e-6, 8e-3, 6.1e-4), "bf16": (7e-7, 2.2e-2, 3e-4)}
T = 0.07
# (37, 40): one tile, padding; (129, 160): a second row tile of one row, 3 16-bit K-steps; (300, 300):
# three column tiles, roundup(d, 128) = 384: the e-chunk edge and a partial chunk
CASES = ([(n, d, "fp32") for n, d in [(37, 40), (129, 160), (300, 300)]]
         + [(n, d, c) for n, d in [(129, 160), (300, 300)] for c in ("fp16", "bf16")] + [(1024, 512, "fp16")])


def _oracle(fn, h, tau):
    x = h.detach().double().requires_grad_(True)
    t = torch.tensor(tau, dtype=torch.float64, device=x.device, requires_grad=True)
    gh, gt = torch.autograd.grad((loss := fn(x, t)), (x, t))
    return loss.item(), gh, gt.item()


def _run(fn, h, tau, compute, **kw):
    x = h.clone().requires_grad_(True)
    t = torch.tensor(tau, dtype=torch.float32, device="cuda", requires_grad=True)
    loss = fn(x, t, compute=compute, **kw)
    loss.backward()
    return loss.detach(), x.grad, t.grad


def _errors(out, ref):
    (loss, dh, dtau), (lref, gref, tref) = out, ref
    return (abs(loss.item() - lref) / max(1.0, abs(lref)), (dh.double() - gref).abs().max().item() / gref.abs().max().item(),
            abs(dtau.item() - tref) / abs(tref))


def _bound(h, tau, compute):
    e_old = _errors(_run(ntxent_amd.ntxent_loss, h, tau, compute), _oracle(R.ntxent_loss, h, tau))
    return tuple(2.0 * max(t, e) for t, e in zip(TABLE[compute], e_old))


@functools.lru_cache(maxsize=None)
def _case(n, d):
    g = torch.Generator().manual_seed(n + d)
    base = torch.randn(n, d, generator=g)
    h = torch.cat([base + 0.3 * torch.randn(n, d, generator=g), base + 0.3 * torch.randn(n, d, generator=g)], 0).cuda()
    return h, _oracle(R.info_nce_loss, h, T)


@pytest.mark.parametrize("n,d,compute", CASES)
def test_parity_with_the_oracle(gpu, n, d, compute):
    h, ref = _case(n, d)
    out = _run(ntxent_amd.info_nce_loss, h, T, compute, backward="fused")
    e, bound = _errors(out, ref), _bound(h, T, compute)
    print(f"XVFUSED n={n} d={d} {compute} loss/dh/dtau={e[0]:.3e}/{e[1]:.3e}/{e[2]:.3e} bound={bound[0]:.3e}/{bound[1]:.3e}/{bound[2]:.3e}")
    assert all(x <= b for x, b in zip(e, bound)), (e, bound)
    assert torch.equal(out[0], _run(ntxent_amd.info_nce_loss, h, T, compute)[0])  # the forward is untouched


@pytest.mark.parametrize("col_splits", [1, 2])
@pytest.mark.parametrize("compute", ["fp32", "fp16"])
def test_column_splits(ext, gpu, compute, col_splits):
    """Three column tiles in one workgroup (persistent accumulators), and shares of 2 and 1."""
    h, ref = _case(300, 300)
    go = torch.ones(1, device="cuda")
    loss, inv, lse2, cpos = ext.xview_forward(h, T, compute)
    dh, dtau = ext.xview_backward_tau(h, inv, lse2, cpos, go, T, compute, fused=True, col_splits=col_splits)
    e, bound = _errors((loss, dh, dtau), ref), _bound(h, T, compute)
    print(f"XVFUSED splits={col_splits} {compute} loss/dh/dtau={e[0]:.3e}/{e[1]:.3e}/{e[2]:.3e}")
    assert all(x <= b for x, b in zip(e, bound)), (e, bound)


@pytest.mark.parametrize("compute", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("n", [37, 200])
def test_orthogonal_rows(gpu, n, compute):
    """One-hot rows: every negative's coefficient is one number, so G rounded to 16 bits once would
    show that rounding undiminished. dh meets the fp32 bound in every compute."""
    v = 3.0 * torch.eye(n, (n + 63) // 64 * 64)
    h = torch.cat([v, v], 0).cuda()
    _, dh, _ = _run(ntxent_amd.info_nce_loss, h, 0.5, compute, backward="fused")
    gref, gt = _oracle(R.info_nce_loss, h, 0.5)[1], _bound(h, 0.5, "fp32")[1]
    ge = (dh.double() - gref).abs().max().item() / gref.abs().max().item()
    print(f"XVFUSED orthogonal n={n} {compute} dh_rel_err={ge:.3e} bound={gt:.3e}")
    assert ge <= gt


@pytest.mark.parametrize("compute", ["fp32", "fp16"])
def test_three_virtual_ranks(gpu, compute):
    """Slot indexing, the own-slot positives and per-slot column padding: every rank's dh against the
    oracle of the global batch in pair order."""
    W, n, d = 3, 70, 72
    g = torch.Generator().manual_seed(7)
    base = torch.randn(W * n, d, generator=g)
    a, b = base + 0.3 * torch.randn(W * n, d, generator=g), base + 0.3 * torch.randn(W * n, d, generator=g)
    shards = [torch.cat([a[r * n:(r + 1) * n], b[r * n:(r + 1) * n]], 0).cuda() for r in range(W)]
    hg = torch.cat([a, b], 0).cuda()
    loss, grads = emulated_xview_forward_backward(shards, T, compute=compute, backward="fused")
    lref, gref, _ = _oracle(R.info_nce_loss, hg, T)
    bound = _bound(hg, T, compute)
    gmax = gref.abs().max().item()
    for r, dh in enumerate(grads):
        want = torch.cat([gref[r * n:(r + 1) * n], gref[W * n + r * n:W * n + (r + 1) * n]], 0)
        ge = (dh.double() - want).abs().max().item() / gmax
        print(f"XVFUSED W=3 rank={r} {compute} dh_rel_err={ge:.3e} bound={bound[1]:.3e}")
        assert ge <= bound[1]
    assert abs(loss.item() - lref) / max(1.0, abs(lref)) <= bound[0]


def test_bitwise_repeatable(gpu):
    h, _ = _case(300, 300)
    a, b = (_run(ntxent_amd.info_nce_loss, h, T, "fp16", backward="fused") for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_backward_peak_memory_below_the_stored_block(gpu):
    """n = 2048, d = 64, fp16: the stored block is 16 MiB, the fused slabs at most 4 x 2 MiB."""
    h = torch.randn(4096, 64, generator=torch.Generator().manual_seed(3)).cuda().half()
    peak = {}
    for mode in ("stored", "fused"):
        x = h.clone().requires_grad_(True)
        loss = ntxent_amd.info_nce_loss(x, T, backward=mode)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss.backward()
        torch.cuda.synchronize()
        peak[mode] = torch.cuda.max_memory_allocated() - base
    print(f"XVFUSED backward peak bytes: stored {peak['stored']} fused {peak['fused']}")
    assert peak["fused"] < peak["stored"]
