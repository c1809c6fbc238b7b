"""ntxent-mi355x: an MI355X-native (gfx950 / CDNA4) NT-Xent (SimCLR) contrastive-loss framework.

Layers: ``csrc/`` (HIP kernels + C++ runtime), ``ops`` (autograd op + oracle),
``parallel`` (RCCL/xGMI global-batch negatives), ``models`` (SimCLR head + synthetic
trainer), ``utils`` (device checks, memory tracking, timing).
"""
__version__ = "0.1.0"

from .ops import (  # noqa: F401,E402
    InfoNCEFunction,
    InfoNCELoss,
    NTXentFunction,
    NTXentLoss,
    SigmoidFunction,
    SigmoidLoss,
    backward,
    check_matrix_core_support,
    check_tensor_core_support,
    contrastive_metrics,
    forward,
    forward_with_stats,
    info_nce_loss,
    ntxent_loss,
    positive_rank,
    sigmoid_loss,
)
