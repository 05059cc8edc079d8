"""Trajectory distances of the flyability evaluation (flyability_utils/trajectory_distances as
flyability_eval.calculate_trajectory_distances calls them) against the reference's own
values (G14, tests/golden/make_golden_traj_dist.py).

The yardstick is `host_distances` below: the 13 metrics in plain numpy, written from their
definitions (tables filled by anti-diagonals, the segment metrics vectorised), in float64 or,
for the golden generator, in np.longdouble.  On CPU the float64 statement is pinned to the
reference's outputs (rtol 1e-12 on the real-valued columns, exact on the count columns EDR /
LCSS); on the GPU the HIP kernels (csrc/tvq_traj.hip) are held to the reference's values.

Bounds.  The generator measures, per column c, gap[c] = max over the golden pairs of
|ref64 - ext| / scale, ext being the longdouble statement: the reference's own rounding error.
The device is held to max(8 gap[c], 64 2^-53) scale: 8 because the device's libm differs from
the host's by a few ulp per call, the floor for columns where the reference happens to hit
the extended value.  scale is |value| except for spherical SSPD / Hausdorff, where it is the
largest great-circle distance within the pair: the bearing difference in the cross-track
distance cancels, so that error is absolute in the distances, not relative to the result.
The four count columns must be exactly equal.  The float32 case is held to
2 |ref32 - ref64| + the float64 bound (as test_stat_metrics.py)."""
import math

import numpy as np
import pytest

from conftest import golden

U = 2.0 ** -53
COLUMNS = ("SSPD Euclidean", "SSPD Spherical", "DTW Euclidean", "DTW Spherical",
           "Hausdorff Euclidean", "Hausdorff Spherical", "LCSS Euclidean", "LCSS Spherical",
           "ERP Euclidean", "ERP Spherical", "EDR Euclidean", "EDR Spherical", "Discrete Frechet")
COUNT_COLS = (6, 7, 10, 11)
SEG_COLS = (0, 1, 4, 5)
TABLE_COLS = tuple(c for c in range(13) if c not in SEG_COLS)
SPH_SEG_COLS = (1, 5)
EPS = 0.009


# ---- the host statement ------------------------------------------------------------------
def _eucl(a, b):
    d0, d1 = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1]
    return np.sqrt(d0 * d0 + d1 * d1)


def _gcd(lon1, lat1, lon2, lat2, T):
    """Haversine great-circle distance, R = 6378137, rad = pi / 180 (the double)."""
    rad, R = T(math.pi / 180.0), T(6378137.0)
    dlat, dlon = rad * (lat2 - lat1), rad * (lon2 - lon1)
    a = (np.sin(dlat / T(2)) * np.sin(dlat / T(2))
         + np.cos(rad * lat1) * np.cos(rad * lat2) * np.sin(dlon / T(2)) * np.sin(dlon / T(2)))
    return R * (T(2) * np.arctan2(np.sqrt(a), np.sqrt(T(1) - a)))


def _bearing(lon1, lat1, lon2, lat2, T):
    rad = T(math.pi / 180.0)
    dlon = rad * (lon2 - lon1)
    y = np.sin(dlon) * np.cos(rad * lat2)
    x = (np.cos(rad * lat1) * np.sin(rad * lat2)
         - np.sin(rad * lat1) * np.cos(rad * lat2) * np.cos(dlon))
    return np.arctan2(y, x)


def _seq_sum(v, T):
    """Python's sum(): left to right."""
    return np.cumsum(np.asarray(v, T))[-1] if len(v) else T(0)


def _sweep(n0, n1, C, cell):
    """Fill C[1:, 1:] by anti-diagonals: C[i, j] = cell(up, left, diag, i, j)."""
    for d in range(2, n0 + n1 + 1):
        i = np.arange(max(1, d - n1), min(n0, d - 1) + 1)
        j = d - i
        C[i, j] = cell(C[i - 1, j], C[i, j - 1], C[i - 1, j - 1], i, j)
    return C[n0, n1]


def _min3(a, b, c):
    return np.minimum(np.minimum(a, b), c)


def host_table(cost, gap0, gap1, eps_edr, eps_lcss, T):
    """(dtw, erp, edr, lcss, discrete frechet) over one cost matrix (n0 x n1)."""
    n0, n1 = cost.shape
    inf = T(np.inf)

    def borders(v0, v1):
        C = np.zeros((n0 + 1, n1 + 1), T)
        C[1:, 0], C[0, 1:] = v0, v1
        return C

    dtw = _sweep(n0, n1, borders(inf, inf),
                 lambda up, lf, dg, i, j: cost[i - 1, j - 1] + _min3(lf, dg, up))
    fre = _sweep(n0, n1, borders(inf, inf),
                 lambda up, lf, dg, i, j: np.maximum(cost[i - 1, j - 1], _min3(lf, dg, up)))
    # every border cell holds the total of all gap distances, not a running sum
    erp = _sweep(n0, n1, borders(_seq_sum(gap0, T), _seq_sum(gap1, T)),
                 lambda up, lf, dg, i, j: _min3(up + gap0[i - 1], lf + gap1[j - 1],
                                                dg + cost[i - 1, j - 1]))
    edr = _sweep(n0, n1, np.zeros((n0 + 1, n1 + 1), np.int64),
                 lambda up, lf, dg, i, j: _min3(
                     lf + 1, up + 1, dg + (~(cost[i - 1, j - 1] < eps_edr)).astype(np.int64)))
    lcss = _sweep(n0, n1, np.zeros((n0 + 1, n1 + 1), np.int64),
                  lambda up, lf, dg, i, j: np.where(cost[i - 1, j - 1] < eps_lcss, dg + 1,
                                                    np.maximum(lf, up)))
    return (dtw, erp, T(int(edr)) / T(max(n0, n1)), T(1) - T(int(lcss)) / T(min(n0, n1)), fre)


def point_to_seg_u(A, B):
    """u of basic_euclidean.point_to_seg for every (point of A, segment of B); nan where the
    segment is degenerate."""
    xd, yd = B[1:, 0] - B[:-1, 0], B[1:, 1] - B[:-1, 1]
    segl = _eucl(B[:-1], B[1:])
    u1 = ((A[:, None, 0] - B[None, :-1, 0]) * xd) + ((A[:, None, 1] - B[None, :-1, 1]) * yd)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((xd == 0) & (yd == 0), np.nan, u1 / (segl * segl))


def _e_directed(A, B, M, T):
    """Per point of A the minimum over B's segments of point_to_seg; M[a, b] = |A[a] - B[b]|."""
    u = point_to_seg_u(A, B)
    xd, yd = B[1:, 0] - B[:-1, 0], B[1:, 1] - B[:-1, 1]
    dps1, dps2 = M[:, :-1], M[:, 1:]
    with np.errstate(invalid="ignore"):
        ix, iy = B[None, :-1, 0] + u * xd, B[None, :-1, 1] + u * yd
        proj = np.sqrt((A[:, None, 0] - ix) ** 2 + (A[:, None, 1] - iy) ** 2)
        d = np.where(np.isnan(u), dps1,
                     np.where((u < T(0.00001)) | (u > T(1)), np.minimum(dps1, dps2), proj))
    return d.min(axis=1)


def _s_directed(A, B, M, T):
    """Per point of A the minimum (from 9e100) over B's segments of point_to_path; M[a, b] the
    great-circle distance of (A[a], B[b])."""
    R = T(6378137.0)
    d12 = _gcd(B[:-1, 0], B[:-1, 1], B[1:, 0], B[1:, 1], T)
    th12 = _bearing(B[:-1, 0], B[:-1, 1], B[1:, 0], B[1:, 1], T)
    th13 = _bearing(B[None, :-1, 0], B[None, :-1, 1], A[:, None, 0], A[:, None, 1], T)
    d13, d23 = M[:, :-1], M[:, 1:]
    with np.errstate(invalid="ignore"):
        crt = np.arcsin(np.sin(d13 / R) * np.sin(th13 - th12)) * R
        d1p = np.arccos(np.cos(d13 / R) / np.cos(crt / R)) * R
        d2p = np.arccos(np.cos(d23 / R) / np.cos(crt / R)) * R
        # a nan along-track distance compares false: |crt| is taken, as in the reference
        ptp = np.where((d1p > d12) | (d2p > d12), np.minimum(d13, d23), np.abs(crt))
    return np.minimum(ptp.min(axis=1), T(9e100))


def host_distances(t0, t1, g, eps=EPS, eps_lcss_s=None, eps_edr_s=None, T=np.float64,
                   segment=True):
    """The 13 distances of one pair in dtype T (segment columns nan when segment is False)."""
    t0, t1 = np.asarray(t0).astype(T), np.asarray(t1).astype(T)
    g = np.asarray(g).astype(T)
    eps_lcss_s = eps * 1e6 if eps_lcss_s is None else eps_lcss_s
    eps_edr_s = eps if eps_edr_s is None else eps_edr_s
    n0, n1 = len(t0), len(t1)
    E = _eucl(t0[:, None, :], t1[None, :, :])
    S = _gcd(t0[:, None, 0], t0[:, None, 1], t1[None, :, 0], t1[None, :, 1], T)
    out = np.full(13, np.nan, T)
    te = host_table(E, _eucl(g[None], t0), _eucl(g[None], t1), T(eps), T(eps), T)
    ts = host_table(S, _gcd(g[0], g[1], t0[:, 0], t0[:, 1], T),
                    _gcd(g[0], g[1], t1[:, 0], t1[:, 1], T), T(eps_edr_s), T(eps_lcss_s), T)
    out[2], out[8], out[10], out[6], out[12] = te
    out[3], out[9], out[11], out[7] = ts[:4]
    if segment:
        e01, e10 = _e_directed(t0, t1, E, T), _e_directed(t1, t0, E.T, T)
        s01, s10 = _s_directed(t0, t1, S, T), _s_directed(t1, t0, S.T, T)
        out[0] = (_seq_sum(e01, T) / T(n0) + _seq_sum(e10, T) / T(n1)) / T(2)
        out[1] = _seq_sum(s10, T) / T(n1) + _seq_sum(s01, T) / T(n0)  # s_sspd does not halve
        out[4] = max(e01.max(), e10.max())
        out[5] = max(s10.max(), s01.max())
    return out


def sph_scale(t0, t1):
    """The largest great-circle distance between a point of t0 and a point of t1."""
    t0, t1 = np.asarray(t0, np.float64), np.asarray(t1, np.float64)
    return float(_gcd(t0[:, None, 0], t0[:, None, 1], t1[None, :, 0], t1[None, :, 1],
                      np.float64).max())


def scales(values, t0, t1):
    """Per column the scale the bounds are relative to."""
    s = np.abs(np.asarray(values, np.float64))
    s[list(SPH_SEG_COLS)] = sph_scale(t0, t1)
    return s


# ---- golden access -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def G():
    d = golden("g14_traj_dist.npz")
    o0, o1 = d["off0"], d["off1"]
    pairs = [(d["pts0"][o0[p]:o0[p + 1]], d["pts1"][o1[p]:o1[p + 1]]) for p in range(len(o0) - 1)]
    return dict(d=d, pairs=pairs, g=tuple(d["g"]), ref=d["ref"], ref_edr_b=d["ref_edr_b"],
                gap=d["gap"], scale=d["scale"], eps_edr_b=float(d["eps_edr_b"]))


def bound(gap, scale):
    return np.maximum(8.0 * gap, 64.0 * U) * scale


def _check(dev, ref, gap, scale, cols, what):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    for c in cols:
        err, lim = abs(dev[c] - ref[c]), bound(gap[c], scale[c])
        print(f"{what} {COLUMNS[c]}: device {dev[c]:.17g} ref {ref[c]:.17g} err {err:.3g} "
              f"bound {lim:.3g}")
        if c in COUNT_COLS:
            assert dev[c] == ref[c], (what, COLUMNS[c], dev[c], ref[c])
        else:
            assert err <= lim, (what, COLUMNS[c], dev[c], ref[c], err, lim)


def _cols_of(t0, t1):
    return range(13) if min(len(t0), len(t1)) >= 2 else TABLE_COLS


# ---- CPU ---------------------------------------------------------------------------------
def test_golden_covers_the_required_lengths(G):
    lens = [(len(a), len(b)) for a, b in G["pairs"]]
    for need in [(1, 1), (1, 5), (5, 1), (2, 2), (2, 3), (63, 64), (64, 65), (65, 63), (130, 257),
                 (257, 130)]:
        assert need in lens
    # a pair longer than the segment kernel's 256-segment tile and several 64-row bands
    assert any(a > 257 for a, _ in lens)
    assert G["gap"].shape == (13,) and (G["gap"][list(COUNT_COLS)] == 0).all()


def test_host_statement_matches_the_reference(G):
    for p, (t0, t1) in enumerate(G["pairs"]):
        seg = min(len(t0), len(t1)) >= 2
        h = host_distances(t0, t1, G["g"], segment=seg)
        cols = _cols_of(t0, t1)
        for c in cols:
            if c in COUNT_COLS:
                assert h[c] == G["ref"][p, c], (p, COLUMNS[c])
            else:
                np.testing.assert_allclose(h[c], G["ref"][p, c], rtol=1e-12, atol=0,
                                           err_msg=f"pair {p} {COLUMNS[c]}")
        hb = host_distances(t0, t1, G["g"], eps_edr_s=G["eps_edr_b"], segment=False)
        assert hb[11] == G["ref_edr_b"][p]
    # the second threshold set makes the spherical EDR column match somewhere
    assert (G["ref_edr_b"] < G["ref"][:, 11]).any()


def test_host_statement_float32_case(G):
    d = G["d"]
    h = host_distances(d["c_t0"].astype(np.float64), d["c_t1"].astype(np.float64), G["g"])
    for c in range(13):
        if c in COUNT_COLS:
            assert h[c] == d["c_out64"][c]
        else:
            np.testing.assert_allclose(h[c], d["c_out64"][c], rtol=1e-12, atol=0)


def test_wrappers_refuse_bad_input():
    from timevqvae.evaluation.flyability_utils import (e_dtw, e_hausdorff, e_sspd, s_hausdorff,
                                                       s_sspd, trajectory_distances_device)
    a, b = np.zeros((3, 2)), np.ones((4, 2))
    with pytest.raises(ValueError, match="2 generated and 1 simulated"):
        trajectory_distances_device([a, a], [b], (0.0, 0.0))
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        trajectory_distances_device([np.zeros((3, 3))], [b], (0.0, 0.0))
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        e_dtw(np.zeros(6), b)
    with pytest.raises(ValueError, match="float32 or float64"):
        trajectory_distances_device([a], [np.ones((4, 2), np.int64)], (0.0, 0.0))
    for f in (e_sspd, s_sspd, e_hausdorff, s_hausdorff):
        with pytest.raises(ValueError, match="at least 2"):
            f(np.zeros((1, 2)), b)
    with pytest.raises(ValueError, match="at least 2"):
        trajectory_distances_device([a], [np.ones((1, 2))], (0.0, 0.0))


def test_exports():
    import timevqvae.evaluation as ev
    from timevqvae.evaluation import flyability_utils as fu
    assert fu.COLUMNS == COLUMNS
    for n in ("e_dtw", "s_dtw", "e_erp", "s_erp", "e_edr", "s_edr", "e_lcss", "s_lcss", "e_sspd",
              "s_sspd", "e_hausdorff", "s_hausdorff", "discret_frechet"):
        assert callable(getattr(fu, n)) and n in fu.__all__
    assert not hasattr(fu, "frechet")
    assert callable(ev.calculate_trajectory_distances)


# ---- GPU ---------------------------------------------------------------------------------
def _batch(gen, sim, g, **kw):
    from timevqvae.evaluation.flyability_utils import trajectory_distances_device
    return trajectory_distances_device(gen, sim, g, **kw)


@pytest.fixture(scope="module")
def dev_rows(G, cuda):
    """Device rows of the golden pairs: the table family on all of them in one ragged batch,
    the segment family on those with two points or more in another."""
    t0s, t1s = [a for a, _ in G["pairs"]], [b for _, b in G["pairs"]]
    out = _batch(t0s, t1s, G["g"], device=cuda, families=("table",)).cpu().numpy()
    long = [p for p, (a, b) in enumerate(G["pairs"]) if min(len(a), len(b)) >= 2]
    full = _batch([t0s[p] for p in long], [t1s[p] for p in long], G["g"], device=cuda).cpu().numpy()
    for k, p in enumerate(long):
        assert np.array_equal(full[k, list(TABLE_COLS)], out[p, list(TABLE_COLS)])
        out[p] = full[k]
    return out, long, full


@pytest.mark.gpu
def test_device_matches_the_reference_on_the_golden_pairs(G, dev_rows):
    out, _, _ = dev_rows
    for p, (t0, t1) in enumerate(G["pairs"]):
        _check(out[p], G["ref"][p], G["gap"], G["scale"][p], _cols_of(t0, t1),
               f"pair {p} {len(t0)}x{len(t1)}")


@pytest.mark.gpu
def test_device_second_threshold_set(G, cuda):
    t0s, t1s = [a for a, _ in G["pairs"]], [b for _, b in G["pairs"]]
    out = _batch(t0s, t1s, G["g"], edr_spherical_eps=G["eps_edr_b"], device=cuda,
                 families=("table",)).cpu().numpy()
    assert np.array_equal(out[:, 11], G["ref_edr_b"])
    for p, (t0, t1) in enumerate(G["pairs"]):
        _check(out[p], G["ref"][p], G["gap"], G["scale"][p], [c for c in TABLE_COLS if c != 11],
               f"set b pair {p}")


@pytest.mark.gpu
def test_device_float32_case(G, cuda):
    d = G["d"]
    assert d["c_t0"].dtype == np.float32
    dev = _batch([d["c_t0"]], [d["c_t1"]], G["g"], device=cuda).cpu().numpy()[0]
    r32, r64 = d["c_out32"], d["c_out64"]
    lim = 2.0 * np.abs(r32 - r64) + bound(G["gap"], d["c_scale"])
    for c in range(13):
        err = abs(dev[c] - r32[c])
        print(f"float32 {COLUMNS[c]}: device {dev[c]:.17g} ref32 {r32[c]:.17g} ref64 "
              f"{r64[c]:.17g} err {err:.3g} bound {lim[c]:.3g}")
        assert err <= lim[c], (COLUMNS[c], dev[c], r32[c], r64[c])
    # the device computes in float64: it meets the float64 reference at the float64 bound
    _check(dev, r64, G["gap"], d["c_scale"], range(13), "float32 widened")
    # a torch float32 tensor on the device takes the same path
    import torch
    dev2 = _batch([torch.from_numpy(d["c_t0"]).to(cuda)], [torch.from_numpy(d["c_t1"])], G["g"])
    assert np.array_equal(dev2.cpu().numpy()[0], dev)


@pytest.mark.gpu
def test_device_rows_do_not_depend_on_the_batch(G, dev_rows, cuda):
    _, long, full = dev_rows
    t0s, t1s = [G["pairs"][p][0] for p in long], [G["pairs"][p][1] for p in long]
    again = _batch(t0s, t1s, G["g"], device=cuda).cpu().numpy()
    assert np.array_equal(again, full)
    for k in range(len(long)):
        alone = _batch([t0s[k]], [t1s[k]], G["g"], device=cuda).cpu().numpy()
        assert np.array_equal(alone[0], full[k]), k
    perm = np.random.default_rng(0).permutation(len(long))
    shuffled = _batch([t0s[k] for k in perm], [t1s[k] for k in perm], G["g"],
                      device=cuda).cpu().numpy()
    assert np.array_equal(shuffled, full[perm])


@pytest.mark.gpu
def test_per_pair_functions_and_dict_equal_the_batch(G, dev_rows, cuda):
    from timevqvae.evaluation import calculate_trajectory_distances
    from timevqvae.evaluation import flyability_utils as fu
    _, long, full = dev_rows
    k = long.index(next(p for p in long if len(G["pairs"][p][0]) == 64))
    t0, t1 = G["pairs"][long[k]]
    g, row = G["g"], full[k]
    got = {"SSPD Euclidean": fu.e_sspd(t0, t1), "SSPD Spherical": fu.s_sspd(t0, t1),
           "DTW Euclidean": fu.e_dtw(t0, t1), "DTW Spherical": fu.s_dtw(t0, t1),
           "Hausdorff Euclidean": fu.e_hausdorff(t0, t1),
           "Hausdorff Spherical": fu.s_hausdorff(t0, t1),
           "LCSS Euclidean": fu.e_lcss(t0, t1, EPS), "LCSS Spherical": fu.s_lcss(t0, t1, EPS * 1e6),
           "ERP Euclidean": fu.e_erp(t0, t1, g), "ERP Spherical": fu.s_erp(t0, t1, g),
           "EDR Euclidean": fu.e_edr(t0, t1, EPS), "EDR Spherical": fu.s_edr(t0, t1, EPS),
           "Discrete Frechet": fu.discret_frechet(t0, t1)}
    for c, name in enumerate(COLUMNS):
        assert type(got[name]) is float and got[name] == row[c], name
    # the table functions take a one-point trajectory
    one = fu.e_dtw(t0[:1], t1[:1])
    assert abs(one - np.hypot(*(t0[0] - t1[0]))) <= 4 * U * one
    t0s, t1s = [G["pairs"][p][0] for p in long], [G["pairs"][p][1] for p in long]
    res = calculate_trajectory_distances(t0s, t1s, g[0], g[1])
    assert list(res) == list(COLUMNS) and "Frechet" not in res
    for c, name in enumerate(COLUMNS):
        assert all(type(v) is float for v in res[name])
        assert res[name] == full[:, c].tolist(), name


@pytest.mark.gpu
def test_device_symmetry(G, dev_rows, cuda):
    _, long, full = dev_rows
    ks = [k for k, p in enumerate(long) if len(G["pairs"][p][0]) in (2, 63, 65)]
    t0s, t1s = [G["pairs"][long[k]][0] for k in ks], [G["pairs"][long[k]][1] for k in ks]
    swapped = _batch(t1s, t0s, G["g"], device=cuda).cpu().numpy()
    checked = set()
    for n, k in enumerate(ks):
        a, b = host_distances(t0s[n], t1s[n], G["g"]), host_distances(t1s[n], t0s[n], G["g"])
        # the host statement decides which metrics are symmetric for this pair
        sym = [c for c in range(13) if (a[c] == b[c] if c in COUNT_COLS
                                        else abs(a[c] - b[c]) <= 1e-12 * abs(a[c]))]
        checked.update(sym)
        _check(swapped[n], G["ref"][long[k]], G["gap"], G["scale"][long[k]], sym, f"swapped {k}")
    assert checked == set(range(13))  # all 13 are symmetric by definition


@pytest.mark.gpu
def test_identical_trajectories_give_zero(G, cuda):
    t = G["pairs"][-1][0]
    out = _batch([t], [t.copy()], G["g"], device=cuda).cpu().numpy()[0]
    for c in (2, 10, 6, 12):
        assert out[c] == 0.0, COLUMNS[c]


@pytest.mark.gpu
def test_device_limits(G, cuda):
    import torch
    from timevqvae.evaluation.flyability_utils import e_dtw
    from timevqvae.hip._native import NativeError, call, ptr, stream_ptr, value
    limit = int(value("tvq_traj_max_len"))
    assert limit >= 4096
    ramp = np.stack([np.linspace(0.1, 0.5, 5), np.linspace(-0.2, 0.3, 5)], axis=1)
    with pytest.raises(ValueError, match="limit"):
        e_dtw(np.zeros((limit + 1, 2)), ramp)
    pts0 = torch.zeros(limit + 1, 2, dtype=torch.float64, device=cuda)
    pts1 = torch.from_numpy(ramp).to(cuda)
    h0, h1 = np.array([0, limit + 1], np.int64), np.array([0, 5], np.int64)
    off0, off1 = torch.from_numpy(h0).to(cuda), torch.from_numpy(h1).to(cuda)
    out = torch.zeros(1, 13, dtype=torch.float64, device=cuda)
    for name, tail in (("tvq_traj_table_distances", (0.0, 0.0, EPS, EPS * 1e6, EPS)),
                       ("tvq_traj_segment_distances", ())):
        with pytest.raises(NativeError, match="the limit is"):  # refused before any launch
            call(name, ptr(pts0), ptr(off0), ptr(pts1), ptr(off1), h0.ctypes.data, h1.ctypes.data,
                 1, *tail, ptr(out), stream_ptr())
    h1[1] = 1  # one point: the segment family refuses, the table family would not
    with pytest.raises(NativeError, match="at least 2"):
        call("tvq_traj_segment_distances", ptr(pts0[:8]), ptr(off1), ptr(pts1), ptr(off1),
             h1.ctypes.data, h1.ctypes.data, 1, ptr(out), stream_ptr())
    torch.cuda.synchronize()
    assert (out == 0).all()
    # exactly at the limit, both ways round: many bands of one wave, and the longest row
    zeros = np.zeros((limit, 2))
    for a, b in ((zeros, ramp), (ramp, zeros)):
        dev = _batch([a], [b], (0.0, 0.0), device=cuda).cpu().numpy()[0]
        host = host_distances(a, b, (0.0, 0.0), segment=False)
        _check(dev, host, G["gap"], scales(host, a, b), (2, 3), f"limit {len(a)}x{len(b)}")


@pytest.mark.gpu
def test_empty_batch(cuda):
    out = _batch([], [], (0.0, 0.0), device=cuda)
    assert tuple(out.shape) == (0, 13) and out.dtype.is_floating_point and out.is_cuda
    from timevqvae.evaluation import calculate_trajectory_distances
    assert calculate_trajectory_distances([], [], 0.0, 0.0) == {n: [] for n in COLUMNS}
