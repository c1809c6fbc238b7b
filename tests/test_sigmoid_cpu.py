"""Pairwise sigmoid loss (the SigLIP form): oracle, analytic gradients, public API, module, trainer
and CLI on the CPU. The GPU kernels are tested in test_gpu_sigmoid.py."""
import math

import pytest
import torch
import torch.nn.functional as F

import ntxent_amd
from ntxent_amd.ops import reference as R

PAIRS = [(0.1, -10.0), (0.5, 0.0)]  # (tau, bias)


def _inputs64(n, dim, seed=0, noise=0.3):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, dim, generator=g, dtype=torch.float64)
    v1 = base + noise * torch.randn(n, dim, generator=g, dtype=torch.float64)
    v2 = base + noise * torch.randn(n, dim, generator=g, dtype=torch.float64)
    return torch.cat([v1, v2], 0)


def _softplus(x):
    return max(x, 0.0) + math.log1p(math.exp(-abs(x)))


@pytest.mark.parametrize("tau,bias", PAIRS)
def test_oracle_is_the_literal_double_loop(tau, bias):
    n = 5
    h = _inputs64(n, 12, seed=1)
    a, b = F.normalize(h[:n], dim=1), F.normalize(h[n:], dim=1)
    want = 0.0
    for i in range(n):
        for j in range(n):
            x = float(a[i] @ b[j]) / tau + bias
            want += _softplus(-x if i == j else x)
    want /= n
    assert abs(R.sigmoid_loss(h, tau, bias).item() - want) <= 1e-13 * max(1.0, want)
    # SigLIP's own expression: -mean over rows of sum_j log sigmoid(s_ij x_ij)
    s = 2.0 * torch.eye(n, dtype=torch.float64) - 1.0
    siglip = -F.logsigmoid(s * (a @ b.t() / tau + bias)).sum() / n
    assert abs(siglip.item() - want) <= 1e-13 * max(1.0, want)


@pytest.mark.parametrize("tau,bias", PAIRS)
def test_analytic_backward_against_autograd(tau, bias):
    h = _inputs64(37, 40, seed=2).requires_grad_(True)
    t = torch.tensor(tau, dtype=torch.float64, requires_grad=True)
    bb = torch.tensor(bias, dtype=torch.float64, requires_grad=True)
    gh, gt, gb = torch.autograd.grad(R.sigmoid_loss(h, t, bb), (h, t, bb))
    for go in (1.0, 3.5):
        dh, dtau, dbias = R.sigmoid_backward_analytic(h.detach(), tau, bias, go)
        assert (dh - go * gh).abs().max().item() <= 1e-12 * max(1.0, go * gh.abs().max().item())
        assert dtau.dim() == 0 and abs(dtau.item() - go * gt.item()) <= 1e-12 * max(1.0, abs(go * gt.item()))
        assert dbias.dim() == 0 and abs(dbias.item() - go * gb.item()) <= 1e-12 * max(1.0, abs(go * gb.item()))


def test_gradcheck():
    h = _inputs64(6, 8, seed=3).requires_grad_(True)
    t = torch.tensor(0.4, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(-1.5, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(R.sigmoid_loss, (h, t, b))


@pytest.mark.parametrize("tau,bias", PAIRS)
@pytest.mark.parametrize("n", [1, 37, 200])
def test_exact_cases(n, tau, bias):
    """One-hot rows: every negative's cosine is 0; identical rows: every cosine is 1."""
    x = 1.0 / tau + bias
    v = 3.0 * torch.eye(n, (n + 63) // 64 * 64, dtype=torch.float64)
    want = _softplus(-x) + (n - 1) * _softplus(bias)
    assert abs(R.sigmoid_loss(torch.cat([v, v], 0), tau, bias).item() - want) <= 1e-13 * max(1.0, want)
    row = torch.randn(40, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    want = _softplus(-x) + (n - 1) * _softplus(x)
    assert abs(R.sigmoid_loss(row.repeat(2 * n, 1), tau, bias).item() - want) <= 1e-13 * max(1.0, want)


def test_public_api_on_cpu():
    h = _inputs64(12, 16, seed=4).float()
    want = R.sigmoid_loss(h, 0.2, -3.0)
    assert torch.equal(ntxent_amd.sigmoid_loss(h, 0.2, -3.0), want)
    assert torch.equal(ntxent_amd.sigmoid_loss(h[:12], 0.2, -3.0, z2=h[12:]), want)
    assert torch.equal(ntxent_amd.SigmoidLoss(0.2, -3.0)(h[:12], h[12:]), want)
    assert torch.equal(ntxent_amd.SigmoidLoss(0.2, -3.0)(h), want)
    assert torch.equal(ntxent_amd.sigmoid_loss(h), R.sigmoid_loss(h, 0.1, -10.0))  # SigLIP's initialisation
    with pytest.raises(ValueError):
        ntxent_amd.sigmoid_loss(h[:23], 0.2)
    with pytest.raises(ValueError):
        ntxent_amd.sigmoid_loss(h, torch.tensor([0.1, 0.2]))
    with pytest.raises(ValueError):
        ntxent_amd.sigmoid_loss(h, 0.1, torch.tensor([0.1, 0.2]))


def test_tensor_temperature_and_bias_get_gradients():
    h = _inputs64(9, 16, seed=6)
    tau = torch.tensor([0.3], dtype=torch.float64, requires_grad=True)
    bias = torch.tensor([[-2.0]], dtype=torch.float64, requires_grad=True)
    a, b = h[:9].clone().requires_grad_(True), h[9:].clone().requires_grad_(True)
    ntxent_amd.sigmoid_loss(a, tau, bias, z2=b).backward()
    dh, dtau, dbias = R.sigmoid_backward_analytic(h, 0.3, -2.0)
    assert tau.grad.shape == tau.shape and bias.grad.shape == bias.shape and bias.grad.dtype == bias.dtype
    assert abs(tau.grad.item() - dtau.item()) <= 1e-12 and abs(bias.grad.item() - dbias.item()) <= 1e-12
    assert torch.allclose(a.grad, dh[:9], rtol=0, atol=1e-12) and torch.allclose(b.grad, dh[9:], rtol=0, atol=1e-12)


def test_module_parameters_bounds_and_repr():
    h = _inputs64(16, 8, seed=7).float()
    m = ntxent_amd.SigmoidLoss()
    assert m.temperature == 0.1 and m.bias == -10.0 and not list(m.parameters())
    assert "temperature=0.1" in m.extra_repr() and "bias=-10.0" in m.extra_repr() and "learnable" not in m.extra_repr()
    m = ntxent_amd.SigmoidLoss(0.5, -1.0, learnable_temperature=True, temperature_bounds=(0.4, 0.6), learnable_bias=True)
    assert sorted(n for n, _ in m.named_parameters()) == ["bias", "log_temperature"]
    assert m.bias.dtype == torch.float32 and m.bias.item() == -1.0
    assert "learnable_temperature=True" in m.extra_repr() and "learnable_bias=True" in m.extra_repr()
    assert abs(m.current_temperature().item() - 0.5) < 1e-7
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    m(h).backward()
    assert m.log_temperature.grad.abs().item() > 0 and m.bias.grad.abs().item() > 0
    opt.step()
    assert abs(m.log_temperature.item() - math.log(0.5)) > 1e-6 and abs(m.bias.item() + 1.0) > 1e-6
    with torch.no_grad():
        m.log_temperature.fill_(math.log(5.0))
    assert abs(m.current_temperature().item() - 0.6) < 1e-7
    only_bias = ntxent_amd.SigmoidLoss(0.5, learnable_bias=True)
    assert [n for n, _ in only_bias.named_parameters()] == ["bias"] and only_bias.bias.item() == -10.0
    with pytest.raises(ValueError):
        ntxent_amd.SigmoidLoss(0.5, learnable_temperature=True, temperature_bounds=(0.0, 1.0))


def _trainer(tmp_path, **kw):
    from ntxent_amd.models.trainer import SimCLRTrainer, TrainConfig

    cfg = TrainConfig(steps=2, batch=16, image_size=8, encoder="mlp", proj_hidden=32, proj_out=16, temperature=0.5,
                      optimizer="lars", lr=0.5, warmup_steps=1, amp=False, log_every=0, ckpt_dir=str(tmp_path),
                      ckpt_every=2, **kw)
    return SimCLRTrainer(cfg, device=torch.device("cpu"))


def test_trainer_sigmoid_with_a_learnable_bias(tmp_path):
    from ntxent_amd.utils.checkpoint import latest_checkpoint

    tr = _trainer(tmp_path, loss="sigmoid", bias=-2.0, learnable_bias=True)
    assert isinstance(tr.loss_fn, ntxent_amd.SigmoidLoss)
    group = tr.opt.param_groups[-1]
    assert group["params"][0] is tr.loss_fn.bias and group["weight_decay"] == 0.0 and group["lars"] is False
    hist = tr.fit()
    assert len(hist) == 2 and all(math.isfinite(r["loss"]) for r in hist)
    assert abs(hist[-1]["bias"] + 2.0) > 1e-6  # the bias moved
    state = torch.load(latest_checkpoint(tmp_path), weights_only=True)
    conf = state["extra"]["config"]
    assert conf["loss"] == "sigmoid" and conf["learnable_bias"] is True and conf["bias"] == -2.0
    assert state["extra"]["bias"] == hist[-1]["bias"]
    again = _trainer(tmp_path, loss="sigmoid", bias=-2.0, learnable_bias=True)  # resumes: the bias comes back
    assert again.step == 2 and abs(again.loss_fn.bias.item() - hist[-1]["bias"]) <= 1e-6


def test_trainer_default_config_saves_the_keys_it_saved(tmp_path):
    from ntxent_amd.utils.checkpoint import latest_checkpoint

    _trainer(tmp_path).fit()
    conf = torch.load(latest_checkpoint(tmp_path), weights_only=True)["extra"]
    assert not {"loss", "bias", "learnable_bias", "learnable_temperature", "metrics_every"} & set(conf["config"])
    assert set(conf) == {"config"}
    with pytest.raises(ValueError):
        _trainer(tmp_path, loss="supcon")
    with pytest.raises(ValueError):
        _trainer(tmp_path, learnable_bias=True)  # the bias belongs to the sigmoid loss


def test_trainer_refuses_sigmoid_at_world_gt_1(tmp_path, monkeypatch):
    from ntxent_amd.models import trainer

    monkeypatch.setattr(trainer, "_dist", lambda: (2, 0))
    with pytest.raises(NotImplementedError, match="one GPU"):
        _trainer(tmp_path, loss="sigmoid")


def test_cli_takes_the_loss_and_the_bias():
    from ntxent_amd.models import train

    ap = train.build_parser()
    cfg = train.config_from_args(ap.parse_args([]))
    assert cfg.loss == "ntxent" and cfg.bias == -10.0 and cfg.learnable_bias is False
    cfg = train.config_from_args(ap.parse_args(["--loss", "sigmoid", "--learnable-bias", "true", "--bias", "-5"]))
    assert cfg.loss == "sigmoid" and cfg.learnable_bias is True and cfg.bias == -5.0
    with pytest.raises(SystemExit):
        ap.parse_args(["--loss", "supcon"])
