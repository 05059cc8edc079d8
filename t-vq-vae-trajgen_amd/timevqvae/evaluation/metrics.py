"""Metrics -- the reference's evaluation/metrics.py:50-214 for the ROCKET feature extractor:
features of the train / test sets, FID between feature sets and the TSGBench statistics.

ROCKET features follow metrics.py:121-124: channel 0, the random kernels, then
F.normalize(p=2, dim=-1) in float32.  One DeviceKernels lives on the instance and the
transform (`apply_kernels_device`), the cast and the normalisation stay on the device; a batch
leaves it once, as float32 numpy.  FID runs `calculate_fid` (device moments) after the
reference's `remove_outliers`; the statistics run timevqvae.evaluation.stat_metrics.

The supervised FCN extractor and the Inception Score are not wired into this class: both
raise NotImplementedError and name the functions of fcn_metrics.py that compute them
(DESIGN.md)."""
from typing import Tuple, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..utils import remove_outliers
from ..utils.sample_utils import conditional_sample, unconditional_sample
from .eval_utils import calculate_fid
from .rocket_functions import DeviceKernels, apply_kernels_device, generate_kernels
from .stat_metrics import stat_metrics_device

FCN_OUT_OF_SCOPE = ("the supervised FCN feature extractor and the Inception Score are not wired "
                    "into this path (DESIGN.md, Out of scope): use timevqvae.evaluation."
                    "load_pretrained_FCN with fcn_features / fcn_inception_score, or "
                    "feature_extractor_type='rocket'")


def rocket_features(x, dk, normalize_dtype):
    """x (b, c, l) numpy or tensor -> (b, 2 * num_kernels) numpy: channel 0 in float64, the
    ROCKET transform, L2-normalised rows in `normalize_dtype`; all on dk's device."""
    xt = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    xt = xt[:, 0, :].to(device=dk.device, dtype=torch.float64)
    z = apply_kernels_device(xt.contiguous(), dk)
    return F.normalize(z.to(normalize_dtype), p=2, dim=-1).cpu().numpy()


def batched(fn, x, batch_size):
    """The reference's batch loop (ragged last batch): fn over slices, concatenated."""
    n = x.shape[0]
    n_iters = n // batch_size + (1 if n % batch_size > 0 else 0)
    return np.concatenate([fn(x[i * batch_size:(i + 1) * batch_size]) for i in range(n_iters)],
                          axis=0)


@torch.no_grad()
def sample(batch_size: int, maskgit, device, n_samples: int, kind: str,
           class_index: Union[None, int]):
    """metrics.py:24-47 -> (x_new_l, x_new_h, x_new), each (b c l)."""
    assert kind in ["unconditional", "conditional"]
    if kind == "unconditional":
        return unconditional_sample(maskgit, n_samples, device, batch_size=batch_size)
    return conditional_sample(maskgit, n_samples, device, class_index, batch_size)


class Metrics(nn.Module):
    def __init__(self, fcn_ckpt_fname, input_length: int, in_channels: int, n_classes: int,
                 batch_size: int, X_train: np.ndarray, X_test: np.ndarray, device,
                 feature_extractor_type: str, rocket_num_kernels: int = 1000):
        super().__init__()
        if feature_extractor_type == "supervised_fcn":
            raise NotImplementedError("Metrics: " + FCN_OUT_OF_SCOPE)
        if feature_extractor_type != "rocket":
            raise ValueError(f"unavailable feature extractor type {feature_extractor_type!r}")
        self.feature_extractor_type = feature_extractor_type
        self.batch_size = batch_size
        self.device = torch.device(device)
        self.X_train = X_train  # (b c l)
        self.X_test = X_test  # (b c l)
        self.n_classes = n_classes
        self.rocket_kernels = generate_kernels(self.X_train.shape[-1], num_kernels=rocket_num_kernels)
        self._device_kernels = DeviceKernels(self.rocket_kernels, self.device)
        self.z_train = self.compute_z(self.X_train)  # (b d)
        self.z_test = self.compute_z(self.X_test)  # (b d)

    @torch.no_grad()
    def sample(self, maskgit, device, n_samples: int, kind: str, class_index: Union[None, int]):
        return sample(self.batch_size, maskgit, device, n_samples, kind, class_index)

    def extract_feature_representations(self, x):
        """x (b c l) -> (b d) float32 numpy."""
        return rocket_features(x, self._device_kernels, torch.float32)

    def compute_z(self, x) -> np.ndarray:
        return batched(self.extract_feature_representations, x, self.batch_size)

    def compute_z_stat(self, x):
        zs = self.compute_z(x)
        return np.mean(zs, axis=0)[None, :], np.std(zs, axis=0)[None, :]  # (1 d), (1 d)

    def z_gen_fn(self, x_gen):
        return self.compute_z(x_gen)

    def fid_score(self, z1: np.ndarray, z2: np.ndarray, sqrtm: str = "host"):
        z1, z2 = remove_outliers(z1), remove_outliers(z2)
        return calculate_fid(z1, z2, self.device, sqrtm=sqrtm)

    def inception_score(self, x_gen):
        raise NotImplementedError("Metrics.inception_score: " + FCN_OUT_OF_SCOPE)

    def stat_metrics(self, x_real, x_gen) -> Tuple[float, float, float, float]:
        """(mdd, acd, sd, kd) of TSGBench (Ang et al., arXiv:2309.03755); x (batch c length)."""
        return tuple(stat_metrics_device(x_real, x_gen, self.device)[:4])
