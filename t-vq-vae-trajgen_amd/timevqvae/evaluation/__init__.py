"""Evaluation on the HIP path: ROCKET features (reference evaluation/rocket_functions.py),
FID / IS (reference evaluation/eval_utils.py; the FID moments on the device, and with
sqrtm="device" / `fid_device` the whole scalar: Jacobi singular values in float64), the TSGBench
statistics MDD / ACD / SD / KD (reference evaluation/stat_metrics.py; KDE, autocorrelation
and central moments on the device) and the `Metrics` class (reference evaluation/metrics.py)
for the ROCKET extractor, and the flyability evaluation's trajectory distances (reference
evaluation/flyability_eval.py calculate_trajectory_distances and flyability_utils/
trajectory_distances; all 14, the continuous Frechet distance included, on the device).  The
supervised FCN extractor (reference models/fcn.py) is in through `load_pretrained_FCN`,
`fcn_features`, `fcn_class_probabilities` and `fcn_inception_score` (fcn_metrics.py; the
eval forward on the device); the string paths (`Metrics(..., "supervised_fcn")`, the sampler's
evaluation half, `.inception_score`) still refuse; the checkpoint it loads is what
trainers.ExpFCN.save writes.  The flyability evaluation's simulation, filtering and plotting
are out of scope."""
from .eval_utils import (calculate_fid, calculate_inception_score, feature_moments,
                         fid_device)
from .fcn_metrics import (fcn_class_probabilities, fcn_features, fcn_inception_score,
                          load_pretrained_FCN)
from .flyability_eval import calculate_trajectory_distances
from .flyability_utils import trajectory_distances_device
from .metrics import Metrics
from .rocket_functions import (DeviceKernels, apply_kernel, apply_kernels, apply_kernels_device,
                               generate_kernels)
from .stat_metrics import (StatMetrics, auto_correlation_difference, kurtosis_difference,
                           marginal_distribution_difference, skewness_difference,
                           stat_metrics_device)

__all__ = ["DeviceKernels", "Metrics", "StatMetrics", "apply_kernel", "apply_kernels",
           "apply_kernels_device", "auto_correlation_difference", "calculate_fid",
           "calculate_inception_score", "calculate_trajectory_distances",
           "fcn_class_probabilities", "fcn_features", "fcn_inception_score", "feature_moments",
           "fid_device", "generate_kernels", "kurtosis_difference", "load_pretrained_FCN",
           "marginal_distribution_difference", "skewness_difference",
           "stat_metrics_device", "trajectory_distances_device"]
