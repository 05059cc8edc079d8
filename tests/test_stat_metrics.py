"""TSGBench statistics MDD / ACD / SD / KD (evaluation/stat_metrics.py:5-60) against the
reference's own values (G13, tests/golden/make_golden_stat.py) and against numpy / scipy.

The yardstick is `host_*` below: the four formulas in plain float64 numpy, written from their
definitions.  On CPU it is pinned to the reference's outputs at rtol 1e-12; on the GPU the
HIP kernels (csrc/tvq_stat.hip) are held to it, to scipy.stats.gaussian_kde and to
np.correlate.  Bounds:

  moments   rtol 1e-10 (float64, another summation order; as test_fid.py); min / max exact
  KDE       per grid point rtol 1e-10 against scipy.stats.gaussian_kde
  MDD       |err| <= 1e-10 x the mean of the two densities (the difference of two densities
            cancels, so the bound is stated on the densities)
  ACF       per lag |err| <= 4 L 2^-53 out[0]: the fp64 summation bound; by Cauchy-Schwarz
            every lag's absolute sum is at most the lag-0 energy
  ACD       the two sets' ACF bounds added
  SD, KD    the moments' 1e-10 carried through m3 / m2^1.5 (2.5e-10 of each |skew|) and
            m4 / m2^2 (3e-10 of each kurtosis + 3)
  float32   |device - ref32| <= 2 |ref32 - ref64| + the float64 bound: the device computes in
            float64 where the reference's float32 path does not, so the reference's own gap
            is the yardstick (the factor 2: the device may sit on the far side of ref64)."""
import numpy as np
import pytest

from conftest import golden

U = 2.0 ** -53


# ---- the float64 statement -------------------------------------------------------------
def host_moments(x):
    """{min, max, mean, m2, m3, m4}: biased central moments about the computed mean."""
    x = np.asarray(x, np.float64).reshape(-1)
    mean = x.sum() / x.size
    d = x - mean
    d2 = d * d
    return np.array([x.min(), x.max(), mean, d2.sum() / x.size, (d2 * d).sum() / x.size,
                     (d2 * d2).sum() / x.size])


def host_bandwidth(x):
    x = np.asarray(x, np.float64).reshape(-1)
    return np.std(x, ddof=1) * x.size ** (-1.0 / 5.0)


def host_kde(x, grid):
    """Gaussian KDE with Scott's bandwidth: whiten, subtract, exp, normalise."""
    x = np.asarray(x, np.float64).reshape(-1)
    s = host_bandwidth(x)
    out = np.empty(len(grid))
    for g, v in enumerate(np.asarray(grid, np.float64)):
        out[g] = np.exp(-0.5 * (v / s - x / s) ** 2).sum()
    return out / (x.size * s * np.sqrt(2.0 * np.pi))


def host_grid(real, gen, points=100):
    return np.linspace(float(min(real.min(), gen.min())), float(max(real.max(), gen.max())), points)


def host_acf(x):
    """Mean over the series of the raw lags 0..L-1 of channel 0."""
    x = np.asarray(x, np.float64)
    L = x.shape[-1]
    return np.mean([np.correlate(s[0], s[0], mode="full")[L - 1:] for s in x], axis=0)


def host_skew_kurt(x, eps=np.finfo(np.float64).eps):
    _, _, mean, m2, m3, m4 = host_moments(x)
    if m2 <= (eps * mean) ** 2:
        return np.nan, np.nan
    return m3 / m2 ** 1.5, m4 / m2 ** 2.0 - 3.0


def host_four(real, gen):
    real, gen = np.asarray(real, np.float64), np.asarray(gen, np.float64)
    grid = host_grid(real, gen)
    mdd = np.mean(np.abs(host_kde(real, grid) - host_kde(gen, grid)))
    acd = np.mean(np.abs(host_acf(real) - host_acf(gen)))
    (skr, kur), (skg, kug) = host_skew_kurt(real), host_skew_kurt(gen)
    return np.array([mdd, acd, abs(skr - skg), abs(kur - kug)])


def float64_bounds(real, gen):
    """The absolute float64 bounds on (mdd, acd, sd, kd) listed in the module docstring."""
    real, gen = np.asarray(real, np.float64), np.asarray(gen, np.float64)
    grid = host_grid(real, gen)
    dens = 0.5 * (host_kde(real, grid).mean() + host_kde(gen, grid).mean())
    L = real.shape[-1]
    (skr, kur), (skg, kug) = host_skew_kurt(real), host_skew_kurt(gen)
    return np.array([1e-10 * dens, 4 * L * U * (host_acf(real)[0] + host_acf(gen)[0]),
                     2.5e-10 * (abs(skr) + abs(skg)), 3e-10 * ((kur + 3.0) + (kug + 3.0))])


def walks(rng, shape, offset=0.0):
    return offset + np.cumsum(rng.standard_normal(shape), axis=-1) * 0.1


# ---- CPU: the statement is the reference ---------------------------------------------------
@pytest.mark.parametrize("k,out", [("a", "a_out"), ("b", "b_out"), ("c", "c_out64")])
def test_host_statement_matches_reference(k, out):
    g = golden("g13_stat.npz")
    np.testing.assert_allclose(host_four(g[f"{k}_real"], g[f"{k}_gen"]), g[out], rtol=1e-12)


def test_golden_holds_a_float32_case():
    g = golden("g13_stat.npz")
    assert g["c_real"].dtype == np.float32 and g["c_gen"].dtype == np.float32
    assert np.array_equal(g["c_real"], g["a_real"].astype(np.float32))
    gap = np.abs(g["c_out32"] - g["c_out64"])
    assert (gap > 0).all() and (gap < 1e-4 * np.abs(g["c_out64"])).all()


# ---- GPU: moments ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 255, 256, 257, 100003])
def test_device_moments(n, cuda):
    import torch
    from timevqvae.evaluation.stat_metrics import moments_device
    x = 3.0 + 0.5 * np.random.default_rng(n).standard_normal(n)
    got = moments_device(torch.from_numpy(x).to(cuda)).cpu().numpy()
    want = host_moments(x)
    print(n, got, want, np.abs(got - want))
    assert got[0] == want[0] and got[1] == want[1]
    np.testing.assert_allclose(got[2:], want[2:], rtol=1e-10, atol=0)


@pytest.mark.gpu
def test_constant_input_gives_nan_skew_and_kurtosis(cuda):
    from timevqvae.evaluation import kurtosis_difference, skewness_difference
    c = np.full((3, 2, 5), 1.7)
    x = walks(np.random.default_rng(0), (4, 2, 5))
    for a, b in ((c, x), (x, c), (c.astype(np.float32), x)):
        assert np.isnan(skewness_difference(a, b)) and np.isnan(kurtosis_difference(a, b))
    assert np.isfinite(skewness_difference(x, x + 1.0))


# ---- GPU: KDE ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("G", [100, 1, 101])
@pytest.mark.parametrize("n", [2, 257, 70001])
def test_device_kde_matches_scipy(n, G, cuda):
    import torch
    from scipy.stats import gaussian_kde
    from timevqvae.evaluation.stat_metrics import kde_device, moments_device, scott_bandwidth
    x = 0.3 + 0.7 * np.random.default_rng(n + G).standard_normal(n)
    grid = np.linspace(x.min(), x.max(), G)
    xt = torch.from_numpy(x).to(cuda)
    s = scott_bandwidth(n, float(moments_device(xt)[3]))
    np.testing.assert_allclose(s, host_bandwidth(x), rtol=1e-10)
    got = kde_device(xt, torch.from_numpy(grid).to(cuda), s).cpu().numpy()
    want = gaussian_kde(x)(grid)
    print(n, G, np.abs(got - want).max() / want.min())
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 257, 70001])
def test_device_mdd_matches_scipy(n, cuda):
    from scipy.stats import gaussian_kde
    from timevqvae.evaluation import marginal_distribution_difference
    rng = np.random.default_rng(n)
    real = (0.3 + 0.7 * rng.standard_normal(n)).reshape(n, 1, 1)
    gen = (0.5 + 0.6 * rng.standard_normal(n + 3)).reshape(n + 3, 1, 1)
    grid = host_grid(real, gen)
    dr, dg = gaussian_kde(real.reshape(-1))(grid), gaussian_kde(gen.reshape(-1))(grid)
    got, want = marginal_distribution_difference(real, gen), np.mean(np.abs(dr - dg))
    print(n, got, want, abs(got - want))
    assert abs(got - want) <= 1e-10 * 0.5 * (dr.mean() + dg.mean())


def test_mdd_refuses_what_scipy_refuses():
    """n < 2 or zero variance: scipy's gaussian_kde raises; so does the bandwidth here."""
    from timevqvae.evaluation.stat_metrics import scott_bandwidth
    for n, m2 in ((1, 0.0), (5, 0.0), (5, float("nan"))):
        with pytest.raises(ValueError):
            scott_bandwidth(n, m2)


# ---- GPU: autocorrelation ------------------------------------------------------------------------
ACF_SHAPES = [(1, 1, 1), (3, 2, 2), (5, 3, 63), (5, 3, 64), (7, 4, 65), (130, 1, 255), (4, 2, 1000),
              (3, 2, 2500), (2, 1, 8192)]  # the last two: several lag tiles; the documented limit


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ACF_SHAPES)
def test_device_acf_matches_numpy(shape, cuda):
    import torch
    from timevqvae.evaluation.stat_metrics import acf_mean_device
    x = walks(np.random.default_rng(sum(shape)), shape, 0.1)
    got = acf_mean_device(torch.from_numpy(x).to(cuda)).cpu().numpy()
    want = host_acf(x)
    L = shape[-1]
    assert got.shape == (L,)
    err = np.abs(got - want).max()
    print(shape, err, 4 * L * U * want[0])
    assert err <= 4 * L * U * want[0]


@pytest.mark.gpu
def test_device_acf_refuses_a_series_above_its_limit(cuda):
    import torch
    from timevqvae.evaluation.stat_metrics import acf_mean_device
    from timevqvae.hip._native import NativeError, call, ptr, stream_ptr, value
    limit = int(value("tvq_stat_acf_max_len"))
    assert limit >= 8192
    x = torch.zeros(2, 1, limit + 1, dtype=torch.float64, device=cuda)
    with pytest.raises(ValueError):
        acf_mean_device(x)
    out = torch.zeros(limit + 1, dtype=torch.float64, device=cuda)
    with pytest.raises(NativeError, match="exceeds the limit"):  # refused before any launch
        call("tvq_stat_acf_mean", ptr(x), 2, limit + 1, limit + 1, ptr(out), ptr(out), stream_ptr())
    torch.cuda.synchronize()


# ---- GPU: the reference's values -------------------------------------------------------------------
def _device_four(real, gen):
    from timevqvae.evaluation import (auto_correlation_difference, kurtosis_difference,
                                      marginal_distribution_difference, skewness_difference)
    return np.array([marginal_distribution_difference(real, gen),
                     auto_correlation_difference(real, gen), skewness_difference(real, gen),
                     kurtosis_difference(real, gen)])


@pytest.mark.gpu
@pytest.mark.parametrize("k", ["a", "b"])
def test_device_metrics_match_reference(k, cuda):
    g = golden("g13_stat.npz")
    real, gen = g[f"{k}_real"], g[f"{k}_gen"]
    got, want, bound = _device_four(real, gen), g[f"{k}_out"], float64_bounds(real, gen)
    print(k, got, want, np.abs(got - want), bound)
    assert all(isinstance(v, float) for v in _device_four(real, gen).tolist())
    assert (np.abs(got - want) <= bound).all()


@pytest.mark.gpu
def test_device_metrics_float32_inputs(cuda):
    g = golden("g13_stat.npz")
    real, gen = g["c_real"], g["c_gen"]
    got = _device_four(real, gen)
    bound = 2 * np.abs(g["c_out32"] - g["c_out64"]) + float64_bounds(real, gen)
    print(got, g["c_out32"], np.abs(got - g["c_out32"]), bound)
    assert (np.abs(got - g["c_out32"]) <= bound).all()


# ---- GPU: behaviour ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stat_metrics_device_is_deterministic_and_consistent(cuda):
    import torch
    from timevqvae.evaluation import stat_metrics_device
    rng = np.random.default_rng(5)
    real, gen = walks(rng, (9, 3, 130)), walks(rng, (11, 3, 130), 0.2)
    a, b = stat_metrics_device(real, gen), stat_metrics_device(real, gen)
    for u, v in zip(a, b):
        if isinstance(u, torch.Tensor):
            assert torch.equal(u, v)
        else:
            assert u == v and isinstance(u, float)
    assert a.grid.shape == (100,) and a.density_real.shape == (100,) and a.acf_gen.shape == (130,)
    assert a.moments_real.shape == (6,)
    np.testing.assert_array_equal(np.array(a[:4]), _device_four(real, gen))
    bound = float64_bounds(real, gen)
    assert (np.abs(np.array(a[:4]) - host_four(real, gen)) <= bound).all()
    # numpy, CPU tensors and device tensors give the same floats
    c = stat_metrics_device(torch.from_numpy(real), torch.from_numpy(gen))
    d = stat_metrics_device(torch.from_numpy(real).to(cuda), torch.from_numpy(gen).to(cuda))
    assert tuple(a[:4]) == tuple(c[:4]) == tuple(d[:4])
    # a non-contiguous view is taken by value, not by layout
    e = stat_metrics_device(torch.from_numpy(real).to(cuda).transpose(0, 1).contiguous().transpose(0, 1),
                            gen)
    assert tuple(e[:4]) == tuple(a[:4])
