"""The ``backward`` keyword of the cross-view InfoNCE entry points, without a GPU."""
import pytest
import torch

import ntxent_amd
from ntxent_amd.parallel import DistInfoNCELoss, dist_info_nce_loss

H = torch.randn(12, 7, generator=torch.Generator().manual_seed(0))


@pytest.mark.parametrize("call", [
    lambda: ntxent_amd.info_nce_loss(H, 0.1, backward="streamed"),
    lambda: ntxent_amd.InfoNCELoss(0.1, backward="streamed"),
    lambda: dist_info_nce_loss(H, 0.1, backward="streamed"),
    lambda: DistInfoNCELoss(0.1, backward="streamed"),
], ids=["info_nce_loss", "InfoNCELoss", "dist_info_nce_loss", "DistInfoNCELoss"])
def test_invalid_backward_raises(call):
    with pytest.raises(ValueError, match="backward"):
        call()


def test_cpu_tensors_give_identical_results():
    out = {}
    for mode in ("stored", "fused"):
        x = H.clone().requires_grad_(True)
        loss = ntxent_amd.InfoNCELoss(0.1, backward=mode)(x)
        loss.backward()
        out[mode] = (loss.detach(), x.grad)
    assert torch.equal(out["stored"][0], out["fused"][0]) and torch.equal(out["stored"][1], out["fused"][1])
    assert "backward=fused" in repr(ntxent_amd.InfoNCELoss(backward="fused"))
    assert "backward" not in repr(ntxent_amd.InfoNCELoss())
