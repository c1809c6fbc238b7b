"""Cross-view InfoNCE (the CLIP-form loss): oracle, analytic gradients, public API and trainer on
the CPU. The GPU kernels are tested in test_gpu_infonce.py."""
import math

import pytest
import torch
import torch.nn.functional as F

import ntxent_amd
from ntxent_amd.ops import reference as R


def _inputs64(n, dim, seed=0, noise=0.3):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, dim, generator=g, dtype=torch.float64)
    v1 = base + noise * torch.randn(n, dim, generator=g, dtype=torch.float64)
    v2 = base + noise * torch.randn(n, dim, generator=g, dtype=torch.float64)
    return torch.cat([v1, v2], 0)


def _clip(h, tau):
    n = h.shape[0] // 2
    a, b = F.normalize(h[:n], dim=1), F.normalize(h[n:], dim=1)
    t = torch.arange(n)
    return 0.5 * F.cross_entropy(a @ b.t() / tau, t) + 0.5 * F.cross_entropy(b @ a.t() / tau, t)


@pytest.mark.parametrize("n", [5, 37, 200])
def test_oracle_is_the_clip_expression(n):
    h = _inputs64(n, 24, seed=n)
    for tau in (0.07, 0.5):
        assert abs(R.info_nce_loss(h, tau).item() - _clip(h, tau).item()) <= 1e-12


@pytest.mark.parametrize("n,tau", [(5, 0.5), (37, 0.07), (200, 0.1)])
def test_analytic_backward_and_temperature_grad(n, tau):
    h = _inputs64(n, 24, seed=n + 1).requires_grad_(True)
    t = torch.tensor(tau, dtype=torch.float64, requires_grad=True)
    gh, gt = torch.autograd.grad(R.info_nce_loss(h, t), (h, t))
    for go in (1.0, 3.5):
        got = R.info_nce_backward_analytic(h.detach(), tau, go)
        assert (got - go * gh).abs().max().item() <= 1e-12 * max(1.0, go * gh.abs().max().item())
        dt = R.info_nce_temperature_grad_analytic(h.detach(), tau, go)
        assert dt.dim() == 0 and abs(dt.item() - go * gt.item()) <= 1e-12 * max(1.0, abs(go * gt.item()))


def test_gradcheck():
    h = _inputs64(3, 5, seed=2).requires_grad_(True)
    t = torch.tensor(0.4, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(R.info_nce_loss, (h, t))


def test_single_pair_is_zero():
    h = _inputs64(1, 8, seed=3)
    assert R.info_nce_loss(h, 0.07).item() == 0.0
    assert R.info_nce_backward_analytic(h, 0.07).abs().max().item() <= 1e-15


def test_public_api_on_cpu():
    h = _inputs64(12, 16, seed=4).float()
    want = R.info_nce_loss(h, 0.2)
    assert torch.equal(ntxent_amd.info_nce_loss(h, 0.2), want)
    assert torch.equal(ntxent_amd.info_nce_loss(h[:12], 0.2, z2=h[12:]), want)
    assert torch.equal(ntxent_amd.InfoNCELoss(0.2)(h[:12], h[12:]), want)
    assert torch.equal(ntxent_amd.InfoNCELoss(0.2)(h), want)
    assert not torch.equal(want, R.ntxent_loss(h, 0.2))  # not NT-Xent
    with pytest.raises(ValueError):
        ntxent_amd.info_nce_loss(h[:23], 0.2)
    with pytest.raises(ValueError):
        ntxent_amd.info_nce_loss(h[0], 0.2)


def test_two_encoders_each_get_their_half():
    h = _inputs64(9, 16, seed=5)
    a, b = h[:9].clone().requires_grad_(True), h[9:].clone().requires_grad_(True)
    ntxent_amd.info_nce_loss(a, 0.3, z2=b).backward()
    g = R.info_nce_backward_analytic(h, 0.3)
    assert torch.allclose(a.grad, g[:9], rtol=0, atol=1e-12) and torch.allclose(b.grad, g[9:], rtol=0, atol=1e-12)


def test_tensor_temperature_gets_a_gradient():
    h = _inputs64(9, 16, seed=6)
    tau = torch.tensor([0.3], dtype=torch.float64, requires_grad=True)
    ntxent_amd.info_nce_loss(h, tau).backward()
    assert tau.grad.shape == tau.shape and tau.grad.dtype == tau.dtype
    assert abs(tau.grad.item() - R.info_nce_temperature_grad_analytic(h, 0.3).item()) <= 1e-12
    ls = torch.tensor(math.log(0.3), dtype=torch.float64, requires_grad=True)
    ntxent_amd.info_nce_loss(h, ls.exp()).backward()  # a grad_fn temperature: chain rule through exp
    assert abs(ls.grad.item() - 0.3 * tau.grad.item()) <= 1e-12
    with pytest.raises(ValueError):
        ntxent_amd.info_nce_loss(h, torch.tensor([0.1, 0.2]))


def test_module_learnable_temperature_trains_and_clamps():
    h = _inputs64(16, 8, seed=7).float()
    m = ntxent_amd.InfoNCELoss(0.5, learnable_temperature=True, temperature_bounds=(0.4, 0.6))
    assert [n for n, _ in m.named_parameters()] == ["log_temperature"]
    assert abs(m.current_temperature().item() - 0.5) < 1e-7
    opt = torch.optim.SGD(m.parameters(), lr=1.0)
    m(h).backward()
    assert m.log_temperature.grad is not None and m.log_temperature.grad.abs().item() > 0
    opt.step()
    assert abs(m.log_temperature.item() - math.log(0.5)) > 1e-6
    with torch.no_grad():
        m.log_temperature.fill_(math.log(5.0))
    assert abs(m.current_temperature().item() - 0.6) < 1e-7
    with torch.no_grad():
        m.log_temperature.fill_(math.log(1e-3))
    assert abs(m.current_temperature().item() - 0.4) < 1e-7
    assert not list(ntxent_amd.InfoNCELoss(0.5).parameters())
    with pytest.raises(ValueError):
        ntxent_amd.InfoNCELoss(0.5, learnable_temperature=True, temperature_bounds=(0.0, 1.0))
    with pytest.raises(TypeError):
        ntxent_amd.InfoNCELoss(0.5, distributed=True)  # no distributed form


def _trainer(tmp_path, **kw):
    from ntxent_amd.models.trainer import SimCLRTrainer, TrainConfig

    cfg = TrainConfig(steps=2, batch=16, image_size=8, encoder="mlp", proj_hidden=32, proj_out=16, temperature=0.5,
                      optimizer="lars", lr=0.5, warmup_steps=1, amp=False, log_every=0, ckpt_dir=str(tmp_path),
                      ckpt_every=2, **kw)
    return SimCLRTrainer(cfg, device=torch.device("cpu"))


def test_trainer_infonce(tmp_path):
    from ntxent_amd.utils.checkpoint import latest_checkpoint

    tr = _trainer(tmp_path, loss="infonce", learnable_temperature=True)
    assert isinstance(tr.loss_fn, ntxent_amd.InfoNCELoss)
    hist = tr.fit()
    assert len(hist) == 2 and all(math.isfinite(r["loss"]) for r in hist)
    assert abs(hist[-1]["temperature"] - 0.5) > 1e-6
    state = torch.load(latest_checkpoint(tmp_path), weights_only=True)
    assert state["extra"]["config"]["loss"] == "infonce"


def test_trainer_default_loss_leaves_the_saved_config_alone(tmp_path):
    from ntxent_amd.utils.checkpoint import latest_checkpoint

    tr = _trainer(tmp_path)
    assert isinstance(tr.loss_fn, ntxent_amd.NTXentLoss)
    tr.fit()
    state = torch.load(latest_checkpoint(tmp_path), weights_only=True)
    assert "loss" not in state["extra"]["config"]
    with pytest.raises(ValueError):
        _trainer(tmp_path, loss="supcon")


def test_trainer_refuses_infonce_at_world_gt_1(tmp_path, monkeypatch):
    from ntxent_amd.models import trainer

    monkeypatch.setattr(trainer, "_dist", lambda: (2, 0))
    with pytest.raises(NotImplementedError, match="one GPU"):
        _trainer(tmp_path, loss="infonce")


def test_cli_takes_the_loss():
    """models/train.py's own parser: --loss ntxent|infonce reaches TrainConfig.loss."""
    from ntxent_amd.models import train

    ap = train.build_parser()
    assert train.config_from_args(ap.parse_args([])).loss == "ntxent"
    assert train.config_from_args(ap.parse_args(["--loss", "ntxent"])).loss == "ntxent"
    cfg = train.config_from_args(ap.parse_args(["--loss", "infonce", "--learnable-temperature", "true",
                                                "--metrics-every", "2"]))
    assert cfg.loss == "infonce" and cfg.learnable_temperature is True and cfg.metrics_every == 2
    with pytest.raises(SystemExit):
        ap.parse_args(["--loss", "supcon"])
