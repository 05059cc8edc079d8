"""Evaluation on the HIP path: ROCKET features (reference evaluation/rocket_functions.py),
FID / IS (reference evaluation/eval_utils.py; the FID moments on the device), the TSGBench
statistics MDD / ACD / SD / KD (reference evaluation/stat_metrics.py; KDE, autocorrelation
and central moments on the device) and the `Metrics` class (reference evaluation/metrics.py)
for the ROCKET extractor.  The supervised FCN feature extractor, and with it the Inception
Score of a trained classifier, is out of scope."""
from .eval_utils import calculate_fid, calculate_inception_score, feature_moments
from .metrics import Metrics
from .rocket_functions import (DeviceKernels, apply_kernel, apply_kernels, apply_kernels_device,
                               generate_kernels)
from .stat_metrics import (StatMetrics, auto_correlation_difference, kurtosis_difference,
                           marginal_distribution_difference, skewness_difference,
                           stat_metrics_device)

__all__ = ["DeviceKernels", "Metrics", "StatMetrics", "apply_kernel", "apply_kernels",
           "apply_kernels_device", "auto_correlation_difference", "calculate_fid",
           "calculate_inception_score", "feature_moments", "generate_kernels",
           "kurtosis_difference", "marginal_distribution_difference", "skewness_difference",
           "stat_metrics_device"]
