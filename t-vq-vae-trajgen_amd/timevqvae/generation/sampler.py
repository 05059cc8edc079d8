"""TrainedModelSampler (reference generation/sampler.py:26-368, without its plots).

Same constructor and `sample(n_samples, kind, class_index)` contract: Stage2 (with its
frozen Stage1) is loaded from the reference's checkpoints, the FidelityEnhancer from
`stage3.ckpt`'s `fidelity_enhancer.*` entries, and sampling runs MaskGIT iterative
decoding, LF/HF decoding and the FidelityEnhancer on the HIP path.

The evaluation half (sampler.py:110-138, 171-368; do_evaluate=True) is there for the ROCKET
feature extractor: `rocket_kernels`, `ts_len`, `n_classes`, `z_train`, `z_test`, the feature
loops `compute_z`, `compute_z_rec`, `compute_z_svq`, `compute_z_gen` (the reference's batch
loop; ROCKET transform and float64 normalisation on the device), `fid_score` and
`stat_metrics` (timevqvae.evaluation).  The supervised FCN extractor and `inception_score`
are not wired into this class (timevqvae.evaluation.fcn_features / fcn_inception_score compute
them) and raise NotImplementedError;
PCA, t-SNE and the log_* plots are not reproduced."""
from typing import Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from ..evaluation.eval_utils import calculate_fid
from ..evaluation.metrics import FCN_OUT_OF_SCOPE, batched, rocket_features
from ..evaluation.rocket_functions import DeviceKernels, generate_kernels
from ..evaluation.stat_metrics import stat_metrics_device
from ..models import FidelityEnhancer
from ..trainers import Stage2
from ..utils import remove_outliers
from ..utils.sample_utils import conditional_sample, unconditional_sample
from ..utils.checkpoint import read_state_dict


class TrainedModelSampler(nn.Module):
    def __init__(self, stage1_ckpt_fname, stage2_ckpt_fname, stage3_ckpt_fname, fcn_ckpt_fname,
                 input_length: int, in_channels: int, n_classes: int, batch_size: int,
                 X_train=None, Y_train=None, X_test=None, Y_test=None, device=None,
                 config: dict = None, use_fidelity_enhancer: bool = True,
                 feature_extractor_type: str = "supervised_fcn", rocket_num_kernels: int = 1000,
                 do_evaluate: bool = True):
        super().__init__()
        assert feature_extractor_type in ["supervised_fcn", "rocket"], \
            "unavailable feature extractor type."
        if do_evaluate and feature_extractor_type == "supervised_fcn":
            raise NotImplementedError("TrainedModelSampler(do_evaluate=True): " + FCN_OUT_OF_SCOPE)
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.config = config
        self.X_train, self.Y_train, self.X_test, self.Y_test = X_train, Y_train, X_test, Y_test
        self.batch_size = batch_size
        self.feature_extractor_type = feature_extractor_type
        self.stage2 = Stage2.load_from_checkpoint(
            stage2_ckpt_fname, stage1_ckpt_fname=stage1_ckpt_fname, fcn_ckpt_fname=fcn_ckpt_fname,
            input_length=input_length, in_channels=in_channels, n_classes=n_classes,
            X_train=X_train, X_test=X_test, config=config, device=device,
            feature_extractor_type=feature_extractor_type, map_location="cpu")
        self.stage2.eval()
        self.maskgit = self.stage2.maskgit
        self.stage1 = self.stage2.maskgit.stage1
        if use_fidelity_enhancer:
            self.fidelity_enhancer = FidelityEnhancer(input_length=input_length,
                                                      in_channels=in_channels, config=config)
            sd = read_state_dict(stage3_ckpt_fname, map_location="cpu")
            self.fidelity_enhancer.load_state_dict(
                {k.replace("fidelity_enhancer.", ""): v for k, v in sd.items()
                 if k.startswith("fidelity_enhancer.")})
            self.fidelity_enhancer.eval()
        else:
            self.fidelity_enhancer = nn.Identity()
        self.to(self.device)
        if do_evaluate:
            self.rocket_kernels = generate_kernels(input_length, num_kernels=rocket_num_kernels)
            self._device_kernels = DeviceKernels(self.rocket_kernels, self.device)
            self.ts_len = self.X_train.shape[-1]  # time series length
            self.n_classes = len(np.unique(self.Y_train))
            self.z_train = self.compute_z("train")
            self.z_test = self.compute_z("test")

    @torch.no_grad()
    def sample(self, n_samples: int, kind: str, class_index: Union[int, None] = None):
        """sampler.py:140-169 -> ((x_new_l, x_new_h, x_new), X_new_R), all (b c l) on host."""
        assert kind in ["unconditional", "conditional"]
        if kind == "unconditional":
            x_new_l, x_new_h, x_new = unconditional_sample(self.maskgit, n_samples, self.device,
                                                           batch_size=self.batch_size)
        else:
            x_new_l, x_new_h, x_new = conditional_sample(self.maskgit, n_samples, self.device,
                                                         class_index, self.batch_size)
        out = []
        for start in range(0, x_new.shape[0], self.batch_size):
            mini = x_new[start:start + self.batch_size]
            out.append(self.fidelity_enhancer(mini.to(self.device)).cpu())
        return (x_new_l, x_new_h, x_new), torch.cat(out)

    # ---- evaluation half (do_evaluate=True, ROCKET features) ----------------------------
    def _extract_feature_representations(self, x):
        """x (b c l) numpy or tensor -> (b d) float64 numpy (sampler.py:185-189): channel 0,
        ROCKET, L2-normalised rows in float64."""
        if not hasattr(self, "_device_kernels"):
            raise RuntimeError("TrainedModelSampler was built with do_evaluate=False")
        return rocket_features(x, self._device_kernels, torch.float64)

    def _set(self, kind: str):
        assert kind in ["train", "test"]
        return self.X_train if kind == "train" else self.X_test

    def compute_z(self, kind: str) -> np.ndarray:
        """Features of X_train / X_test (sampler.py:278-304)."""
        return batched(self._extract_feature_representations, self._set(kind), self.batch_size)

    @torch.no_grad()
    def compute_z_rec(self, kind: str) -> np.ndarray:
        """Features of the stage-1 reconstructions of X_train / X_test (sampler.py:194-227)."""
        def one(x):
            x = torch.as_tensor(x).float().to(self.device)
            x_rec = self.stage1.forward(batch=(x, None), batch_idx=-1, return_x_rec=True)
            return self._extract_feature_representations(x_rec)
        return batched(one, self._set(kind), self.batch_size)

    @torch.no_grad()
    def compute_z_svq(self, kind: str):
        """(features, X') of the stochastic variant X' of X_train / X_test: tokens drawn with
        svq_temp = the FidelityEnhancer's tau, decoded (sampler.py:229-276)."""
        xs_a = []

        def one(x):
            x = torch.as_tensor(x).float().to(self.device)
            tau = self.fidelity_enhancer.tau.item()
            _, s_a_l = self.maskgit.encode_to_z_q(x, self.stage1.encoder_l, self.stage1.vq_model_l,
                                                  svq_temp=tau)
            _, s_a_h = self.maskgit.encode_to_z_q(x, self.stage1.encoder_h, self.stage1.vq_model_h,
                                                  svq_temp=tau)
            x_a = (self.maskgit.decode_token_ind_to_timeseries(s_a_l, "lf")
                   + self.maskgit.decode_token_ind_to_timeseries(s_a_h, "hf"))  # (b c l)
            xs_a.append(x_a.cpu().numpy().astype(float))
            return self._extract_feature_representations(x_a)
        zs = batched(one, self._set(kind), self.batch_size)
        return zs, np.concatenate(xs_a, axis=0)

    def compute_z_gen(self, X_gen: torch.Tensor) -> np.ndarray:
        """Features of generated samples (sampler.py:306-327)."""
        return batched(self._extract_feature_representations, X_gen, self.batch_size)

    def fid_score(self, z1: np.ndarray, z2: np.ndarray, sqrtm: str = "host"):
        z1, z2 = remove_outliers(z1), remove_outliers(z2)
        return calculate_fid(z1, z2, self.device, sqrtm=sqrtm)

    def inception_score(self, X_gen):
        raise NotImplementedError("TrainedModelSampler.inception_score: " + FCN_OUT_OF_SCOPE)

    def stat_metrics(self, x_real, x_gen) -> Tuple[float, float, float, float]:
        """(mdd, acd, sd, kd) of TSGBench (Ang et al., arXiv:2309.03755); x (batch c length)."""
        return tuple(stat_metrics_device(x_real, x_gen, self.device)[:4])
