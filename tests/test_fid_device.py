"""FID end to end on the device (evaluation.fid_device, calculate_fid(sqrtm="device");
csrc/tvq_fid_sqrt.hip): tr sqrtm(sigma1 sigma2) as the sum of the singular values of A1 A2^T
by one-sided Jacobi in float64.

Fixture G16 (tests/golden/make_golden_fid_device.py): per case z1, z2, `ref` (the reference's
calculate_fid), `lap` (the same scalar from numpy.linalg.svd of A1 A2^T), `tr` = tr sigma1 +
tr sigma2 and `ref_gap` = |ref - lap|.  Tolerances:
  * against LAPACK 1e-12 tr: n r eps with n, r <= 300 vectors / rotations a vector, times 10;
  * against the reference 4 ref_gap + 1e-12 tr: the reference's own measured distance from the
    exact statement (its sqrtm of a singular product is off by ~1e-8 tr on the few cases), with
    a factor 4 because that distance moves with LAPACK's rounding from machine to machine;
  * the kernel alone against numpy.linalg.svd: 1e-13 s_max sqrt(n m) on the sorted values.
"""
import functools

import numpy as np
import pytest

from conftest import golden
from fid_jacobi_model import fid_jacobi, fid_lapack

FEW = ["few_a", "few_const", "few_square", "few_same", "few_tiny", "few_f32"]
MANY = ["many_edge", "many_a", "many_graded", "many_const", "many_same"]
CASES = FEW + MANY


@functools.lru_cache(maxsize=None)
def fixture():
    g = golden("g16_fid_device.npz")
    assert list(g["names"]) == CASES
    return {k: g[k] for k in g.files}


def case(k):
    g = fixture()
    return g[f"{k}_z1"], g[f"{k}_z2"]


@functools.lru_cache(maxsize=None)
def device_run(k, form="auto", swap=False, max_sweeps=40):
    """(fid, out (5,), info (5,)) of fid_device on fixture case k, computed once."""
    from timevqvae.evaluation import fid_device
    z1, z2 = case(k)
    if swap:
        z1, z2 = z2, z1
    fid, out, info = fid_device(z1, z2, form=form, max_sweeps=max_sweeps, return_parts=True)
    return float(fid), out.cpu().numpy(), info.cpu().numpy()


# ------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("k", CASES)
def test_numpy_jacobi_fid_matches_lapack(k):
    g = fixture()
    z1, z2 = case(k)
    fid, tr, sweeps, ok = fid_jacobi(z1, z2)
    assert ok and max(sweeps) <= 20, sweeps
    assert (sweeps[0] == 0) == (k in FEW)
    np.testing.assert_allclose(tr, g[f"{k}_tr"], rtol=1e-13)
    assert abs(fid - g[f"{k}_lap"]) <= 1e-12 * g[f"{k}_tr"]


def test_calculate_fid_refuses_unknown_sqrtm():
    from timevqvae.evaluation import calculate_fid
    z = np.zeros((4, 3))
    with pytest.raises(ValueError, match="sqrtm"):
        calculate_fid(z, z, sqrtm="bogus")


def test_sqrtm_keywords_default_to_the_host_path():
    import inspect
    from timevqvae.evaluation import Metrics, calculate_fid
    from timevqvae.generation import TrainedModelSampler
    from timevqvae.trainers import Stage3
    for fn, name in ((calculate_fid, "sqrtm"), (Metrics.fid_score, "sqrtm"),
                     (TrainedModelSampler.fid_score, "sqrtm"),
                     (Stage3.search_optimal_tau, "fid_sqrtm")):
        assert inspect.signature(fn).parameters[name].default == "host", fn


# ------------------------------------------------------- GPU: tvq_jacobi_sv alone
def _sv(a, m_dot=None, max_sweeps=40):
    import torch
    from timevqvae.hip.linalg import jacobi_sv
    t = torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()
    sigma, info = jacobi_sv(t, m_dot, max_sweeps)
    return sigma.cpu().numpy(), info.cpu().numpy(), t.cpu().numpy()


def _check_sv(a):
    n, m = a.shape
    want = np.sort(np.linalg.svd(a, compute_uv=False))
    if n > len(want):  # more vectors than the rank allows: the rest are zero
        want = np.concatenate([np.zeros(n - len(want)), want])
    sigma, info, rot = _sv(a)
    assert info[1] == 1 and 1 <= info[0] <= 40, info
    tol = 1e-13 * want.max() * np.sqrt(n * m)
    err = np.abs(np.sort(sigma) - want).max()
    print(f"jacobi_sv {a.shape}: sweeps {info[0]} err {err:.3e} tol {tol:.3e}")
    assert err <= tol
    return sigma, rot


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(1, 7), (2, 3), (5, 4), (33, 47), (64, 64)])
def test_jacobi_sv_matches_lapack(cuda, n, m):
    a = np.random.default_rng(100 * n + m).standard_normal((n, m))
    sigma, rot = _check_sv(a)
    if n <= m:  # the rows are orthogonal afterwards
        gram = rot @ rot.T
        off = gram - np.diag(np.diag(gram))
        assert np.abs(off).max() <= 1e-13 * np.sqrt(m) * sigma.max() ** 2


@pytest.mark.gpu
def test_jacobi_sv_rank_deficient(cuda):
    rng = np.random.default_rng(20)
    _check_sv(rng.standard_normal((65, 20)) @ rng.standard_normal((20, 130)))


@pytest.mark.gpu
def test_jacobi_sv_degenerate_inputs(cuda):
    rng = np.random.default_rng(21)
    a = rng.standard_normal((9, 12))
    a[4] = 0.0
    sigma, rot = _check_sv(a)
    assert sigma[4] == 0.0 and not rot[4].any()  # a zero vector is never touched
    a = rng.standard_normal((9, 12))
    a[6] = a[2]
    _check_sv(a)
    a = rng.standard_normal((8, 12))
    a[[1, 2]] *= 1e-80
    a[[5, 6]] *= 1e80
    sigma, _ = _check_sv(a)
    # nothing overflowed, and each scale keeps its own values: 2 tiny, 4 of order one, 2 huge
    # (a row scaling D B with cond(B) far below 1e3 moves no value out of its decade band)
    s = np.sort(sigma)
    assert np.isfinite(s).all()
    assert (s[:2] > 1e-83).all() and (s[:2] < 1e-77).all()
    assert (s[2:6] > 1e-3).all() and (s[2:6] < 1e3).all()
    assert (s[6:] > 1e77).all() and (s[6:] < 1e83).all()


@pytest.mark.gpu
def test_jacobi_sv_stacked_mode_gives_the_eigensystem(cuda):
    rng = np.random.default_rng(22)
    D = 48
    b = rng.standard_normal((D, 60))
    s = b @ b.T / 60
    s = (s + s.T) / 2
    sigma, info, rot = _sv(np.concatenate([s, np.eye(D)], 1), m_dot=D)
    assert info[1] == 1
    lam = np.linalg.eigvalsh(s)
    assert np.abs(np.sort(sigma) - lam).max() <= 1e-13 * lam.max() * D
    V = rot[:, D:].T  # columns v_j
    assert np.abs(V.T @ V - np.eye(D)).max() <= 1e-13
    assert np.abs(s @ V - V * sigma[None, :]).max() <= 1e-13 * lam.max() * D
    # the top block is sigma V itself
    assert np.abs(rot[:, :D].T - s @ V).max() <= 1e-13 * lam.max() * D


@pytest.mark.gpu
def test_jacobi_sv_and_fid_device_are_run_to_run_identical(cuda):
    a = np.random.default_rng(23).standard_normal((33, 47))
    r1, r2 = _sv(a), _sv(a)
    for x, y in zip(r1, r2):
        np.testing.assert_array_equal(x, y)
    from timevqvae.evaluation import fid_device
    for k in ("few_a", "many_a"):
        again = fid_device(*case(k), return_parts=True)[1].cpu().numpy()
        np.testing.assert_array_equal(again, device_run(k)[1])


@pytest.mark.gpu
def test_jacobi_sv_not_converged_is_nan(cuda):
    a = np.random.default_rng(24).standard_normal((33, 47))
    sigma, info, _ = _sv(a, max_sweeps=1)
    assert np.isnan(sigma).all() and list(info) == [1, 0]


@pytest.mark.gpu
def test_jacobi_sv_refuses_bad_arguments(cuda):
    import torch
    from timevqvae.hip._native import NativeError
    from timevqvae.hip.linalg import jacobi_sv
    a = torch.zeros(4, 6, dtype=torch.float64, device=cuda)
    with pytest.raises(NativeError, match="max_sweeps"):
        jacobi_sv(a, max_sweeps=65)
    with pytest.raises(NativeError, match="m_dot"):
        jacobi_sv(a, m_dot=7)
    with pytest.raises(ValueError):
        jacobi_sv(a.float())


# ------------------------------------------------------- GPU: fid_device on the fixture
@pytest.mark.gpu
@pytest.mark.parametrize("k", CASES)
def test_fid_device_matches_lapack_and_reference(cuda, k):
    """Measured on an MI355X, |dev - lap| / tr: few 0, 0, 5.0e-16, 2.2e-16, 0, 3.3e-16; many 0,
    1.7e-16, 8.2e-16, 1.7e-16, 1.1e-15.

    The last assertion (on every few case the device is no further from lap than the reference)
    is sharp on few_square (48, 70, 48): sigma2 is regular there and the reference's sqrtm is
    itself accurate to rounding, |ref - lap| = 7.1e-15 = 2.6e-15 tr.  It caught the rotation in
    its plain form c x_p - s x_q, whose c rounds up to 1 at small angles and inflated every
    singular value by 10 - 30 ulps over 11 sweeps (|dev - lap| = 9.8e-15); the kernel rotates in
    Rutishauser's form since (csrc/tvq_fid_sqrt.hip) and is at 1.3e-15."""
    g = fixture()
    fid, out, info = device_run(k)
    lap, ref, tr, gap = (float(g[f"{k}_{n}"]) for n in ("lap", "ref", "tr", "ref_gap"))
    print(f"{k}: dev {fid:.17g} |dev-lap|/tr {abs(fid - lap) / tr:.2e} |dev-ref|/tr "
          f"{abs(fid - ref) / tr:.2e} ref_gap/tr {gap / tr:.2e} info {info.tolist()}")
    assert info[0] == (1 if k in FEW else 2) and info[4] == 1
    assert (info[1] == 0 and info[2] == 0) == (k in FEW) and 1 <= info[3] <= 40
    assert fid == out[0] and out[0] == ((out[1] + out[2]) + out[3]) - 2.0 * out[4]
    np.testing.assert_allclose(out[2] + out[3], tr, rtol=1e-12)
    assert abs(fid - lap) <= 1e-12 * tr
    assert abs(fid - ref) <= 4.0 * gap + 1e-12 * tr
    if k in FEW:
        assert abs(fid - lap) <= abs(ref - lap)


@pytest.mark.gpu
@pytest.mark.parametrize("k,rtol", [("a", 1e-9), ("b", 1e-9), ("c", 1e-5)])
def test_fid_device_matches_g10(cuda, k, rtol):
    from timevqvae.evaluation import calculate_fid
    g = golden("g10_fid.npz")
    fid = calculate_fid(g[f"{k}_z1"], g[f"{k}_z2"], sqrtm="device")
    assert isinstance(fid, float)
    np.testing.assert_allclose(fid, g[f"{k}_fid"], rtol=rtol)


# ------------------------------------------------------------------ GPU: further checks
@pytest.mark.gpu
@pytest.mark.parametrize("k", ["few_same", "many_same"])
def test_fid_device_identical_sets_is_zero(cuda, k):
    assert abs(device_run(k)[0]) <= 1e-12 * float(fixture()[f"{k}_tr"])


@pytest.mark.gpu
@pytest.mark.parametrize("k", ["few_a", "few_f32", "many_a", "many_graded"])
def test_fid_device_swapped_arguments_agree(cuda, k):
    assert abs(device_run(k)[0] - device_run(k, swap=True)[0]) <= 1e-12 * float(fixture()[f"{k}_tr"])


@pytest.mark.gpu
def test_fid_device_forced_forms_agree(cuda):
    tr = float(fixture()["many_a_tr"])
    many, few = device_run("many_a"), device_run("many_a", form="few")
    assert many[2][0] == 2 and few[2][0] == 1 and few[2][4] == 1
    assert abs(many[0] - few[0]) <= 1e-12 * tr


@pytest.mark.gpu
def test_fid_device_tile_edge_shape(cuda):
    """(N1, N2, D) = (300, 257, 513): every extent one past a multiple of the 64 x 64 product
    tile or the 32-deep K stage, 257 vectors (an odd count: a bye in every round)."""
    from timevqvae.evaluation import fid_device
    rng = np.random.default_rng(25)
    z1 = rng.standard_normal((300, 513))
    z2 = 1.3 * rng.standard_normal((257, 513)) + 0.2
    lap, tr = fid_lapack(z1, z2)
    fid, out, info = fid_device(z1, z2, return_parts=True)
    info = info.cpu().numpy()
    print(f"tile edge: |dev-lap|/tr {abs(float(fid) - lap) / tr:.2e} info {info.tolist()}")
    assert info[0] == 1 and info[4] == 1
    assert abs(float(fid) - lap) <= 1e-12 * tr


@pytest.mark.gpu
def test_fid_device_not_converged_is_nan_and_raises(cuda, monkeypatch):
    from timevqvae.evaluation import eval_utils
    fid, out, info = device_run("few_a", max_sweeps=1)
    assert np.isnan(fid) and np.isnan(out[4]) and info[4] == 0 and info[3] == 1
    assert np.isfinite(out[1:4]).all()
    real = eval_utils.fid_device
    monkeypatch.setattr(eval_utils, "fid_device",
                        lambda z1, z2, device=None: real(z1, z2, device, max_sweeps=1))
    with pytest.raises(RuntimeError, match="converge"):
        eval_utils.calculate_fid(*case("few_a"), sqrtm="device")


@pytest.mark.gpu
def test_fid_device_input_kinds_and_argument_checks(cuda):
    import torch
    from timevqvae.evaluation import fid_device
    z1, z2 = case("few_f32")
    want = device_run("few_f32")[0]
    got = fid_device(torch.from_numpy(z1).cuda(), torch.from_numpy(z2), device=cuda)
    assert got.is_cuda and got.dim() == 0 and got.dtype == torch.float64
    assert float(got) == want
    assert float(fid_device(z1.astype(np.float64), z2.astype(np.float64))) == want
    with pytest.raises(ValueError, match="form"):
        fid_device(z1, z2, form="some")
    with pytest.raises(ValueError):
        fid_device(z1, z2[:, :5])
    with pytest.raises(ValueError, match="2048"):
        fid_device(np.zeros((4, 2049)), np.zeros((4, 2049)))


@pytest.mark.gpu
def test_calculate_fid_default_is_the_host_path_bit_for_bit(cuda):
    from scipy.linalg import sqrtm
    from timevqvae.evaluation import calculate_fid, feature_moments
    z1, z2 = case("many_a")
    (mu1, s1), (mu2, s2) = feature_moments(z1), feature_moments(z2)
    mu1, mu2, s1, s2 = (t.cpu().numpy() for t in (mu1, mu2, s1, s2))
    cm = sqrtm(s1.dot(s2))
    want = ((mu1 - mu2) ** 2.0).sum() + np.trace(s1 + s2 - 2.0 * (cm.real if np.iscomplexobj(cm) else cm))
    assert calculate_fid(z1, z2) == want
    assert calculate_fid(z1, z2, sqrtm="host") == want
    assert calculate_fid(z1, z2, cuda) == want


@pytest.mark.gpu
def test_metrics_fid_score_passes_sqrtm_through(cuda):
    from timevqvae.evaluation import Metrics, calculate_fid
    from timevqvae.utils import remove_outliers
    rng = np.random.default_rng(26)
    X = np.cumsum(rng.standard_normal((12, 1, 32)), -1)
    np.random.seed(0)
    m = Metrics(None, 32, 1, 2, 8, X, X[:6], cuda, "rocket", rocket_num_kernels=4)
    z1, z2 = case("few_const")
    want = calculate_fid(remove_outliers(z1), remove_outliers(z2), sqrtm="device")
    assert m.fid_score(z1, z2, sqrtm="device") == want
    assert m.fid_score(z1, z2) == calculate_fid(remove_outliers(z1), remove_outliers(z2))
    assert abs(m.fid_score(z1, z2) - want) <= 1e-6 * float(fixture()["few_const_tr"])
