"""Learnable temperature without a GPU: the closed form of d loss / d tau against autograd
through the fp64 oracle, the ``NTXentLoss(learnable_temperature=True)`` module on CPU inputs, the
refusal of the distributed paths, and the trainer option."""
import math

import pytest
import torch

from ntxent_amd.ops import reference as R


def _inputs64(rows, dim, seed=0, noise=0.3):
    # (tests/test_gpu_kernels._inputs without the device copy)
    g = torch.Generator().manual_seed(seed)
    n = rows // 2
    base = torch.randn(n, dim, generator=g, dtype=torch.float64)
    v1 = base + noise * torch.randn(n, dim, generator=g, dtype=torch.float64)
    v2 = base + noise * torch.randn(n, dim, generator=g, dtype=torch.float64)
    return torch.cat([v1, v2], 0)


def _autograd_dtau(h, T):
    tau = torch.tensor(T, dtype=torch.float64, requires_grad=True)
    (d,) = torch.autograd.grad(R.ntxent_loss(h, tau), tau)
    return d.item()


@pytest.mark.parametrize("T", [0.07, 0.5, 1.0])
@pytest.mark.parametrize("rows,dim", [(64, 128), (34, 100), (600, 200)])
def test_analytic_matches_autograd(rows, dim, T):
    h = _inputs64(rows, dim, seed=rows + dim)
    ref = _autograd_dtau(h, T)
    got = R.ntxent_temperature_grad_analytic(h, T)
    assert got.dim() == 0 and got.dtype == torch.float64
    assert abs(got.item() - ref) <= 1e-10 * abs(ref), (got.item(), ref)
    # scales with grad_out (a float or a tensor)
    assert abs(R.ntxent_temperature_grad_analytic(h, T, 3.5).item() - 3.5 * ref) <= 1e-10 * abs(3.5 * ref)
    g = torch.tensor(-0.25, dtype=torch.float64)
    assert abs(R.ntxent_temperature_grad_analytic(h, T, g).item() + 0.25 * ref) <= 1e-10 * abs(0.25 * ref)


def test_module_learnable_temperature_cpu():
    from ntxent_amd import NTXentLoss

    h = _inputs64(64, 48, seed=1)
    m = NTXentLoss(0.2, learnable_temperature=True)
    assert isinstance(m.log_temperature, torch.nn.Parameter) and m.log_temperature.dtype == torch.float32
    assert list(m.state_dict()) == ["log_temperature"]
    assert abs(m.log_temperature.item() - math.log(0.2)) < 1e-7
    x = h.clone().requires_grad_(True)
    m(x).backward()
    tau = math.exp(m.log_temperature.item())  # the fp32 parameter's value
    ref = _autograd_dtau(h, tau) * tau        # d/d log tau = tau d/d tau
    assert m.log_temperature.grad is not None and m.log_temperature.grad.dtype == torch.float32
    assert abs(m.log_temperature.grad.item() - ref) <= 1e-5 * abs(ref), (m.log_temperature.grad.item(), ref)
    # dh is that of the same temperature as a float
    y = h.clone().requires_grad_(True)
    R.ntxent_loss(y, tau).backward()
    assert torch.allclose(x.grad, y.grad, rtol=1e-5, atol=1e-9)
    assert "learnable_temperature=True" in repr(m)


def test_module_temperature_bounds_clamp():
    from ntxent_amd import NTXentLoss

    h = _inputs64(32, 16, seed=2)
    m = NTXentLoss(0.5, learnable_temperature=True, temperature_bounds=(0.1, 0.3))
    assert abs(m.current_temperature().item() - 0.3) < 1e-7  # above the upper bound
    loss = m(h)
    assert abs(loss.item() - R.ntxent_loss(h, m.current_temperature().item()).item()) < 1e-9
    loss.backward()
    assert m.log_temperature.grad.item() == 0.0  # clamped: no gradient flows
    with torch.no_grad():
        m.log_temperature.fill_(math.log(0.001))
    assert abs(m.current_temperature().item() - 0.1) < 1e-7
    with pytest.raises(ValueError):
        NTXentLoss(0.5, learnable_temperature=True, temperature_bounds=(0.0, 1.0))


def test_module_option_off_is_unchanged():
    from ntxent_amd import NTXentLoss

    m = NTXentLoss(0.07)
    assert len(m.state_dict()) == 0 and not list(m.parameters())
    assert repr(m) == "NTXentLoss(temperature=0.07, compute=auto, distributed=False)"
    assert m.current_temperature() == 0.07


def test_functional_tensor_temperature_cpu():
    """A tensor temperature is no longer detached: autograd through the oracle path carries its
    gradient, also through log_scale.exp()."""
    import ntxent_amd

    h = _inputs64(34, 20, seed=3)
    log_s = torch.tensor(math.log(0.3), dtype=torch.float64, requires_grad=True)
    ntxent_amd.ntxent_loss(h, log_s.exp()).backward()
    ref = _autograd_dtau(h, 0.3) * 0.3
    assert log_s.grad is not None and abs(log_s.grad.item() - ref) <= 1e-9 * abs(ref)
    with pytest.raises(ValueError):
        ntxent_amd.ntxent_loss(h, torch.tensor([0.1, 0.2]))


def test_distributed_paths_refuse_temperature_grad():
    from ntxent_amd import NTXentLoss
    from ntxent_amd.parallel.distributed import cpu_dist_ntxent_loss, dist_ntxent_loss
    from ntxent_amd.parallel.engine_loss import engine_ntxent_loss
    from ntxent_amd.parallel.ring import ring_ntxent_loss
    from ntxent_amd.parallel.symmetric import cpu_sym_ntxent_loss, sym_ntxent_loss

    h = _inputs64(16, 8).float()
    tau = torch.tensor(0.1, requires_grad=True)
    derived = torch.tensor(math.log(0.1)).requires_grad_(True).exp()  # has a grad_fn
    for t in (tau, derived):
        for fn in (dist_ntxent_loss, cpu_dist_ntxent_loss, ring_ntxent_loss, sym_ntxent_loss, cpu_sym_ntxent_loss,
                   engine_ntxent_loss):
            with pytest.raises(NotImplementedError, match="requires grad"):
                fn(h, t)
        for neg in ("allgather", "symmetric", "ring"):
            with pytest.raises(NotImplementedError, match="requires grad"):
                dist_ntxent_loss(h, t, negatives=neg, impl="torch")
    with pytest.raises(NotImplementedError, match="one GPU"):
        NTXentLoss(0.1, distributed=True, learnable_temperature=True)


def test_native_engine_refuses_temperature_grad_at_world_gt_1():
    from ntxent_amd.parallel.native import NativeNTXent

    with pytest.raises(NotImplementedError, match="one GPU"):
        NativeNTXent(512, 128, 0.1, world=2, rank=0, temperature_grad=True)


def _trainer(tmp_path, **kw):
    from ntxent_amd.models.trainer import SimCLRTrainer, TrainConfig

    cfg = TrainConfig(steps=3, batch=16, image_size=8, encoder="mlp", proj_hidden=32, proj_out=16, temperature=0.5,
                      optimizer="lars", lr=0.5, warmup_steps=1, amp=False, log_every=0, ckpt_dir=str(tmp_path),
                      ckpt_every=3, **kw)
    return SimCLRTrainer(cfg, device=torch.device("cpu"))


def test_trainer_learnable_temperature(tmp_path):
    from ntxent_amd.utils.checkpoint import latest_checkpoint

    tr = _trainer(tmp_path, learnable_temperature=True)
    grp = tr.opt.param_groups[-1]  # a group of its own: no weight decay, no LARS adaptation
    assert grp["params"][0] is tr.loss_fn.log_temperature and len(grp["params"]) == 1
    assert grp["weight_decay"] == 0.0 and grp["lars"] is False
    hist = tr.fit()
    assert len(hist) == 3 and all("temperature" in r for r in hist)
    t_end = tr.loss_fn.current_temperature().item()
    assert hist[-1]["temperature"] == t_end and abs(t_end - 0.5) > 1e-6  # three steps moved it
    state = torch.load(latest_checkpoint(tmp_path), weights_only=True)
    assert abs(state["extra"]["log_temperature"] - tr.loss_fn.log_temperature.item()) < 1e-7
    assert state["extra"]["config"]["learnable_temperature"] is True
    # a new trainer resumes the temperature (and the step) from the checkpoint
    tr2 = _trainer(tmp_path, learnable_temperature=True)
    assert tr2.step == 3
    assert tr2.loss_fn.log_temperature.item() == tr.loss_fn.log_temperature.item()


def test_trainer_option_off_is_unchanged(tmp_path):
    from ntxent_amd.utils.checkpoint import latest_checkpoint

    tr = _trainer(tmp_path)
    assert len(tr.opt.param_groups) == 2 and not list(tr.loss_fn.parameters())
    hist = tr.fit()
    assert set(hist[0]) == {"step", "loss", "lr", "step_ms", "images_per_s"}
    state = torch.load(latest_checkpoint(tmp_path), weights_only=True)
    assert set(state["extra"]) == {"config"} and "learnable_temperature" not in state["extra"]["config"]
    assert float(tr.loss_fn.current_temperature()) == 0.5


def test_trainer_refuses_learnable_temperature_at_world_gt_1(tmp_path, monkeypatch):
    from ntxent_amd.models import trainer

    monkeypatch.setattr(trainer, "_dist", lambda: (2, 0))
    with pytest.raises(NotImplementedError, match="one GPU"):
        _trainer(tmp_path, learnable_temperature=True)
