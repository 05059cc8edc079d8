"""TSGBench statistics -- the API of the reference timevqvae/evaluation/stat_metrics.py
(marginal_distribution_difference, auto_correlation_difference, skewness_difference,
kurtosis_difference; :5-60) with the sums on the device.

The reference runs scipy.stats.gaussian_kde (100 grid points against every sample),
np.correlate per series and scipy.stats.skew / kurtosis on one host core.  Here the inputs
(numpy arrays or torch tensors, CPU or CUDA, float32 or float64, (N, C, L)) are moved to the
device as float64 once and csrc/tvq_stat.hip does the O(n) and O(N L^2) work in float64:

  MDD  everything flattened; a 100-point np.linspace grid between the smaller minimum and the
       larger maximum (endpoints as Python floats: a float64 grid); two Gaussian KDEs with
       Scott's bandwidth std(ddof=1) n^(-1/5) (tvq_stat_kde); mean |difference|.
  ACD  channel 0 only (the reference takes series[0]); the mean over the series of the raw
       lags np.correlate(s, s, "full")[L - 1:] (tvq_stat_acf_mean); mean |difference|.
  SD   |skew_r - skew_g|, skew = m3 / m2^1.5      } biased central moments about the mean
  KD   |kurt_r - kurt_g|, kurt = m4 / m2^2 - 3    } (tvq_stat_moments), nan where scipy's are

`stat_metrics_device` returns the four from one upload together with the intermediates.
There is no CPU fallback."""
from collections import namedtuple

import numpy as np
import torch

from ..hip._native import call, ptr, stream_ptr, value
from ._device import resolve_device

GRID_POINTS = 100

StatMetrics = namedtuple("StatMetrics", ["mdd", "acd", "sd", "kd", "grid", "density_real",
                                         "density_gen", "acf_real", "acf_gen", "moments_real",
                                         "moments_gen"])


def _upload(a, device=None):
    """(float64 contiguous (N, C, L) tensor on the device, eps of the input's dtype)."""
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    if t.dim() != 3:
        raise ValueError(f"stat_metrics: expected (N, C, L), got {tuple(t.shape)}")
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"stat_metrics: expected float32 or float64, got {t.dtype}")
    eps = float(torch.finfo(t.dtype).eps)
    dev = resolve_device(device, (t,))
    # copy in the input's dtype, widen on the device: a float32 set crosses the bus once, as is
    return t.detach().to(dev).to(torch.float64).contiguous(), eps


def _ws(name, x, *args):
    return torch.empty(max(int(value(name, *args)), 1), dtype=torch.float64, device=x.device)


def moments_device(x):
    """out6 = {min, max, mean, m2, m3, m4} (float64 device tensor) of every element of x."""
    n = x.numel()
    if n < 1:
        raise ValueError("stat_metrics: empty input")
    out6 = torch.empty(6, dtype=torch.float64, device=x.device)
    ws = _ws("tvq_stat_moments_workspace", x, n)
    call("tvq_stat_moments", ptr(x), n, ptr(out6), ptr(ws), stream_ptr())
    return out6


def kde_device(x, grid, s):
    """gaussian_kde(x)(grid) for a flat float64 device tensor x and bandwidth s."""
    n, G = x.numel(), grid.numel()
    out = torch.empty(G, dtype=torch.float64, device=x.device)
    ws = _ws("tvq_stat_kde_workspace", x, n, G)
    call("tvq_stat_kde", ptr(x), n, ptr(grid), G, float(s), ptr(out), ptr(ws), stream_ptr())
    return out


def acf_mean_device(x):
    """Mean raw autocorrelation (L,) of channel 0 of a contiguous float64 (N, C, L) tensor."""
    N, C, L = x.shape
    if N < 1 or L < 1:
        raise ValueError("stat_metrics: empty input")
    limit = int(value("tvq_stat_acf_max_len"))
    if L > limit:
        raise ValueError(f"stat_metrics: series length {L} exceeds the ACF kernel's limit {limit}")
    out = torch.empty(L, dtype=torch.float64, device=x.device)
    ws = _ws("tvq_stat_acf_workspace", x, N, L)
    call("tvq_stat_acf_mean", ptr(x), N, C * L, L, ptr(out), ptr(ws), stream_ptr())
    return out


def scott_bandwidth(n, m2):
    """std(ddof=1) n^(-1/5): gaussian_kde's default factor for d = 1."""
    if n < 2:
        raise ValueError("`dataset` input should have multiple elements.")
    if not m2 > 0.0:
        raise ValueError("stat_metrics: the KDE needs data of non-zero variance")
    return float(np.sqrt(m2 * n / (n - 1.0)) * np.power(float(n), -0.2))


def _skew_kurt(m, eps):
    """(skew, kurtosis) from out6 on the host; nan where scipy's are (m2 <= (eps mean)^2)."""
    mean, m2, m3, m4 = m[2], m[3], m[4], m[5]
    if m2 <= (eps * mean) ** 2:
        return float("nan"), float("nan")
    return float(m3 / m2 ** 1.5), float(m4 / m2 ** 2.0 - 3.0)


def _mdd(xr, xg, mr, mg):
    lo, hi = min(float(mr[0]), float(mg[0])), max(float(mr[1]), float(mg[1]))
    sr, sg = scott_bandwidth(xr.numel(), float(mr[3])), scott_bandwidth(xg.numel(), float(mg[3]))
    grid = torch.from_numpy(np.linspace(lo, hi, GRID_POINTS)).to(xr.device)
    dr, dg = kde_device(xr.reshape(-1), grid, sr), kde_device(xg.reshape(-1), grid, sg)
    return float((dr - dg).abs().mean()), grid, dr, dg


def _acd(xr, xg):
    if xr.shape[-1] != xg.shape[-1]:
        raise ValueError(f"auto_correlation_difference: series lengths differ "
                         f"({xr.shape[-1]} and {xg.shape[-1]})")
    ar, ag = acf_mean_device(xr), acf_mean_device(xg)
    return float((ar - ag).abs().mean()), ar, ag


def stat_metrics_device(real, generated, device=None):
    """(mdd, acd, sd, kd) and the intermediates (grid, both densities, both lag vectors, both
    out6) as a StatMetrics tuple, from one upload of each set."""
    (xr, er), (xg, eg) = _upload(real, device), _upload(generated, device)
    m6r, m6g = moments_device(xr), moments_device(xg)
    mr, mg = m6r.cpu().numpy(), m6g.cpu().numpy()
    mdd, grid, dr, dg = _mdd(xr, xg, mr, mg)
    acd, ar, ag = _acd(xr, xg)
    (skr, kur), (skg, kug) = _skew_kurt(mr, er), _skew_kurt(mg, eg)
    return StatMetrics(mdd, acd, float(abs(skr - skg)), float(abs(kur - kug)), grid, dr, dg, ar, ag,
                       m6r, m6g)


def marginal_distribution_difference(real, generated):
    (xr, _), (xg, _) = _upload(real), _upload(generated)
    mr, mg = moments_device(xr).cpu().numpy(), moments_device(xg).cpu().numpy()
    return _mdd(xr, xg, mr, mg)[0]


def auto_correlation_difference(real, generated):
    (xr, _), (xg, _) = _upload(real), _upload(generated)
    return _acd(xr, xg)[0]


def _moment_pair(real, generated):
    (xr, er), (xg, eg) = _upload(real), _upload(generated)
    return (_skew_kurt(moments_device(xr).cpu().numpy(), er),
            _skew_kurt(moments_device(xg).cpu().numpy(), eg))


def skewness_difference(real, generated):
    (skr, _), (skg, _) = _moment_pair(real, generated)
    return float(abs(skr - skg))


def kurtosis_difference(real, generated):
    (_, kur), (_, kug) = _moment_pair(real, generated)
    return float(abs(kur - kug))
