"""The supervised FCN extractor's half of the evaluation (reference evaluation/eval_utils.py
load_pretrained_FCN, evaluation/metrics.py:107-120 and :180-199): the 128-d pooled features
that FID is taken of, the class probabilities, and the Inception Score of those.

The FCN's eval forward runs on the HIP path (timevqvae.models.FCNBaseline); a batch is
uploaded once and its result downloaded once.  A sample's row does not depend on the batch it
is in.  The features plug in wherever a feature function is taken:
`Stage3.search_optimal_tau(feature_fn=lambda X: fcn_features(fcn, X, batch_size))`,
`calculate_fid(fcn_features(...), fcn_features(...))`.
"""
import numpy as np
import torch

from ..hip import fcn as ops
from ..models.fcn import FCNBaseline
from .eval_utils import calculate_inception_score
from .metrics import batched


def load_pretrained_FCN(ckpt_fname: str, in_channels: int, n_classes: int):
    """The reference's `torch.save(fcn.state_dict())` checkpoint -> FCNBaseline on the CPU, in
    eval mode, parameters frozen; move it with `.to(device)`."""
    fcn = FCNBaseline(in_channels, n_classes)
    fcn.load_state_dict(torch.load(ckpt_fname, weights_only=True, map_location="cpu"))
    fcn.eval()
    for p in fcn.parameters():
        p.requires_grad_(False)
    return fcn


def _device_batch(fcn, x):
    device = next(fcn.parameters()).device
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return xt.to(device=device, dtype=torch.float32)


def fcn_features(fcn, x, batch_size: int) -> np.ndarray:
    """x (n, c, l) numpy or tensor of any float dtype -> (n, 128) float32 numpy."""
    return batched(lambda xb: ops.fcn_forward(fcn, _device_batch(fcn, xb), True).cpu().numpy(),
                   x, batch_size)


def fcn_class_probabilities(fcn, x, batch_size: int) -> np.ndarray:
    """x (n, c, l) -> softmax of the FCN's logits, (n, classes) float32 numpy."""
    def probs(xb):
        return ops.fcn_forward(fcn, _device_batch(fcn, xb), return_probs=True)[1].cpu().numpy()
    return batched(probs, x, batch_size)


def fcn_inception_score(fcn, x_gen, batch_size: int, n_split: int = 5):
    """(mean, std) of the Inception Score of the FCN's class probabilities on x_gen
    (reference Metrics.inception_score: n_split = 5, rows shuffled with np.random)."""
    return calculate_inception_score(fcn_class_probabilities(fcn, x_gen, batch_size),
                                     n_split=n_split)
