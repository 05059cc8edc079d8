"""FCNBaseline -- the reference's supervised feature extractor (models/fcn.py, from
arXiv:1909.04939 via okrasolar/pytorch-timeseries) as a parameter holder with the reference's
state-dict keys, its eval forward (timevqvae.hip.fcn) and its training step
(timevqvae.hip.fcn_train) on the HIP path.

ConvBlock(in, 128, 8) -> ConvBlock(128, 256, 5) -> ConvBlock(256, 128, 3) -> mean over
positions -> Linear(128, classes); every conv is TensorFlow-"same" padded, stride 1.  `forward`
is the eval forward and refuses training mode; training goes through `loss(x, y)`, the
cross-entropy of the training-mode network with its gradients (trainers.ExpFCN drives it).
"""
import torch
from torch import nn

from ..hip import fcn as ops
from ..hip import fcn_train


class ConvBlock(nn.Module):
    """Conv1d ("same" padding) -> BatchNorm1d -> ReLU; `layers.0` / `layers.1` hold the
    parameters (fcn.py:42-62), the arithmetic is one tvq_fcn_conv_bn_relu launch."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, stride: int) -> None:
        super().__init__()
        assert stride == 1, "the HIP path has the FCN's stride-1 blocks only"
        self.layers = nn.Sequential(
            nn.Conv1d(in_channels, out_channels, kernel_size, stride=stride),
            nn.BatchNorm1d(num_features=out_channels),
            nn.ReLU(),
        )


class FCNBaseline(nn.Module):
    def __init__(self, in_channels: int, num_pred_classes: int = 1) -> None:
        super().__init__()
        self.input_args = {"in_channels": in_channels, "num_pred_classes": num_pred_classes}
        self.layers = nn.Sequential(
            ConvBlock(in_channels, 128, 8, 1),
            ConvBlock(128, 256, 5, 1),
            ConvBlock(256, 128, 3, 1),
        )
        self.final = nn.Linear(128, num_pred_classes)

    def forward(self, x: torch.Tensor, return_feature_vector: bool = False) -> torch.Tensor:
        """x (b, c, l) -> logits (b, classes), or the (b, 128) pooled features.  Eval mode
        only (training mode raises NotImplementedError), under no_grad, input cast to fp32."""
        return ops.fcn_forward(self, x, return_feature_vector)

    def loss(self, x: torch.Tensor, y: torch.Tensor):
        """Training mode: (loss, logits) = (CrossEntropyLoss()(fcn(x), y), fcn(x)) with batch
        statistics; loss.backward() gives the parameters' gradients and the running statistics
        are updated (hip.fcn_train.fcn_loss).  y: int64 class indices (b,) or (b, 1)."""
        return fcn_train.fcn_loss(self, x, y)

    def train(self, mode: bool = True):
        """nn.Module.train, and the eval path's cached fold of the BatchNorm statistics is
        dropped: the training kernels and the fused optimizer write through raw pointers, which
        moves neither `data_ptr` nor `_version`."""
        self.__dict__.pop("_fcn_fold", None)
        return super().train(mode)
