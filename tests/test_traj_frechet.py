"""The continuous Frechet distance (flyability_utils/trajectory_distances/frechet.py, the 14th
distance of flyability_eval.calculate_trajectory_distances) against the reference's own
values (G15, tests/golden/make_golden_frechet.py).

The yardstick is `host_frechet` below: the reference's algorithm in vectorised numpy with the
device's operation order (plain + - * / sqrt, every distance as sqrt(dx dx + dy dy)), in
float64 or, for the golden generator, in np.longdouble.  It returns the value and the trace
of probe outcomes of the binary search.  On CPU the float64 statement is pinned to the
reference's values; on the GPU the HIP kernels (csrc/tvq_traj_frechet.hip) are held to the
reference's values.

Bound.  The generator measures gap = the largest, over the golden pairs and relative to
scale = |ext| (ext the np.longdouble statement), of |ref - ext|, |ref - host64| and
|host64 - host64 with mdist, P_dist and Q_dist moved by +-1 ulp| (4 seeds): the reference's
own rounding freedom, none of it from the device.  Everything is held to
bound(gap, scale) = max(8 gap, 64 2^-53) scale, the rule of tests/test_traj_dist.py.  The
generator also asserts that the critical values next to the answer's cluster (values equal
within 1e-12) lie at least 1e-9 away, so a single wrong probe is an error of 1e-9 or more."""
import numpy as np
import pytest

from conftest import golden

U = 2.0 ** -53
LENGTHS = [(1, 1), (1, 5), (5, 1), (2, 2), (2, 3), (3, 2), (63, 64), (64, 65), (65, 63),
           (130, 257), (257, 130)]
CONSTRUCTED = ("identical", "end moved", "repeated points", "vertical run in Q",
               "vertical run in P", "float32 values")
KEYS14 = ("SSPD Euclidean", "SSPD Spherical", "DTW Euclidean", "DTW Spherical",
          "Hausdorff Euclidean", "Hausdorff Spherical", "LCSS Euclidean", "LCSS Spherical",
          "ERP Euclidean", "ERP Spherical", "EDR Euclidean", "EDR Spherical", "Discrete Frechet",
          "Frechet")


# ---- the host statement ------------------------------------------------------------------
def _dist(ax, ay, bx, by):
    dx, dy = ax - bx, ay - by
    return np.sqrt(dx * dx + dy * dy)


def _point_to_seg(px, py, p1x, p1y, p2x, p2y, dps1, dps2, segl, T):
    """basic_euclidean.point_to_seg, elementwise."""
    deg = (p1x == p2x) & (p1y == p2y)
    xd, yd = p2x - p1x, p2y - p1y
    u1 = ((px - p1x) * xd) + ((py - p1y) * yd)
    with np.errstate(all="ignore"):
        u = u1 / (segl * segl)
        ix, iy = p1x + u * xd, p1y + u * yd
        proj = _dist(px, py, ix, iy)
        ends = (u < T(0.00001)) | (u > T(1))
    return np.where(deg, dps1, np.where(ends, np.where(dps2 < dps1, dps2, dps1), proj))


def _free_line(px, py, s1x, s1y, s2x, s2y, dps1, dps2, ds, eps, T):
    """frechet.free_line with circle_line_intersection inlined, elementwise: (lo, hi)."""
    zero, one, none = T(0), T(1), T(-1)
    deg = (s1x == s2x) & (s1y == s2y)
    pts = _point_to_seg(px, py, s1x, s1y, s2x, s2y, dps1, dps2, ds, T)
    segl2 = ds * ds
    vert = s2x == s1x
    with np.errstate(all="ignore"):
        rac = np.sqrt((eps * eps) - ((s1x - px) * (s1x - px)))
        m = (s2y - s1y) / (s2x - s1x)
        c = s2y - m * s2x
        A = m * m + one
        B = T(2) * (((m * c) - (m * py)) - px)
        C = ((((py * py) - (eps * eps)) + (px * px)) - ((T(2) * c) * py)) + (c * c)
        delta = (B * B) - ((T(4) * A) * C)
        tang = delta <= zero
        sd = np.sqrt(np.where(tang, zero, delta))
        xt = (-B) / (T(2) * A)
        x1 = np.where(vert, s1x, np.where(tang, xt, ((-B) + sd) / (T(2) * A)))
        x2 = np.where(vert, s1x, np.where(tang, xt, ((-B) - sd) / (T(2) * A)))
        y1 = np.where(vert, py + rac, m * x1 + c)
        y2 = np.where(vert, py - rac, m * x2 + c)
        differ = (x1 != x2) | (y1 != y2)
        u1 = (((x1 - s1x) * (s2x - s1x)) + ((y1 - s1y) * (s2y - s1y))) / segl2
        u2 = (((x2 - s1x) * (s2x - s1x)) + ((y2 - s1y) * (s2y - s1y))) / segl2
        # sorted((0, 1, u1, u2))[1:3]
        lo_u, hi_u = np.where(u2 < u1, u2, u1), np.where(u2 < u1, u1, u2)
        a, b = np.where(lo_u > zero, lo_u, zero), np.where(hi_u < one, hi_u, one)
        lo_d, hi_d = np.where(b < a, b, a), np.where(b < a, a, b)
        at1, at2 = (px == s1x) & (py == s1y), (px == s2x) & (py == s2y)
        single = np.where(at1, zero, np.where(at2, one, np.where((zero <= u1) & (u1 <= one), u1, none)))
        far = pts > eps
    lo = np.where(deg, np.where(dps1 > eps, none, zero),
                  np.where(far, none, np.where(differ, lo_d, single)))
    hi = np.where(deg, np.where(dps1 > eps, none, one),
                  np.where(far, none, np.where(differ, hi_d, single)))
    return lo, hi


class _Pair:
    """The reference's setup: mdist, P_dist, Q_dist (optionally each moved by +-1 ulp)."""

    def __init__(self, P, Q, T, ulp_seed=None):
        self.T = T
        self.P, self.Q = np.asarray(P).astype(T), np.asarray(Q).astype(T)
        P, Q = self.P, self.Q
        self.p, self.q = len(P), len(Q)
        self.M = _dist(P[:, None, 0], P[:, None, 1], Q[None, :, 0], Q[None, :, 1])
        self.Pd = _dist(P[:-1, 0], P[:-1, 1], P[1:, 0], P[1:, 1])
        self.Qd = _dist(Q[:-1, 0], Q[:-1, 1], Q[1:, 0], Q[1:, 1])
        if ulp_seed is not None:
            rng = np.random.default_rng(ulp_seed)
            for name in ("M", "Pd", "Qd"):
                v = getattr(self, name)
                to = np.where(rng.integers(0, 2, v.shape) == 1, T(np.inf), T(-np.inf))
                setattr(self, name, np.where(v > 0, np.nextafter(v, to), v))

    def L(self):  # (p - 1, q - 1): point_to_seg(Q[j], P[i], P[i + 1], ...)
        P, Q, M = self.P, self.Q, self.M
        return _point_to_seg(Q[None, :-1, 0], Q[None, :-1, 1], P[:-1, None, 0], P[:-1, None, 1],
                             P[1:, None, 0], P[1:, None, 1], M[:-1, :-1], M[1:, :-1],
                             self.Pd[:, None], self.T)

    def B(self):  # (p - 1, q - 1): point_to_seg(P[i], Q[j], Q[j + 1], ...)
        P, Q, M = self.P, self.Q, self.M
        return _point_to_seg(P[:-1, None, 0], P[:-1, None, 1], Q[None, :-1, 0], Q[None, :-1, 1],
                             Q[None, 1:, 0], Q[None, 1:, 1], M[:-1, :-1], M[:-1, 1:],
                             self.Qd[None, :], self.T)

    def LF(self, eps):  # (p - 1, q) intervals
        P, Q, M = self.P, self.Q, self.M
        return _free_line(Q[None, :, 0], Q[None, :, 1], P[:-1, None, 0], P[:-1, None, 1],
                          P[1:, None, 0], P[1:, None, 1], M[:-1, :], M[1:, :], self.Pd[:, None],
                          eps, self.T)

    def BF(self, eps):  # (p, q - 1) intervals
        P, Q, M = self.P, self.Q, self.M
        return _free_line(P[:, None, 0], P[:, None, 1], Q[None, :-1, 0], Q[None, :-1, 1],
                          Q[None, 1:, 0], Q[None, 1:, 1], M[:, :-1], M[:, 1:], self.Qd[None, :],
                          eps, self.T)

    def critical_values(self):
        end_point = max(self.M[0, 0], self.M[-1, -1])
        if self.p < 2 or self.q < 2:
            return np.array([end_point], self.T)
        L, B = self.L(), self.B()
        return np.unique(np.concatenate([[end_point], L[L > end_point], B[B > end_point]]))

    def decide(self, eps):
        """frechet.decision_problem."""
        p, q = self.p, self.q
        lfl, lfh = self.LF(eps)
        bfl, bfh = self.BF(eps)
        if not (lfl[0, 0] <= 0 and bfl[0, 0] <= 0 and lfh[p - 2, q - 1] >= 1
                and bfh[p - 1, q - 2] >= 1):
            return False
        lf_some, bf_some = ~((lfl == -1) & (lfh == -1)), ~((bfl == -1) & (bfh == -1))
        lf_full, bf_full = (lfl == 0) & (lfh == 1), (bfl == 0) & (bfh == 1)
        col0 = np.ones(p - 1, bool)   # LR[(i, 0)]
        col0[1:] = lf_some[1:, 0] & lf_full[:-1, 0]
        row0 = np.ones(q - 1, bool)   # BR[(0, j)]
        row0[1:] = bf_some[0, 1:] & bf_full[0, :-1]
        idx = np.arange(q - 1)
        reach = None
        for i in range(p - 1):
            seed = row0.copy() if i == 0 else reach & bf_some[i, :q - 1]
            seed[0] |= col0[i]
            # reach[j] = seed[j] or (lf_some[i, j] and reach[j - 1]): the last seed at or before
            # j is not before the last column that blocks
            block = ~lf_some[i, :q - 1]
            block[0] = True
            last_seed = np.maximum.accumulate(np.where(seed, idx, -1))
            last_block = np.maximum.accumulate(np.where(block, idx, -1))
            reach = last_seed >= last_block
        return bool(reach[q - 2])


def host_frechet(P, Q, T=np.float64, ulp_seed=None):
    """(frechet(P, Q), trace): the value in dtype T and the outcome of every probe."""
    pair = _Pair(P, Q, T, ulp_seed)
    cc = pair.critical_values()
    eps, first, n, trace = cc[0], 0, len(cc), []
    while n != 1:
        m = int(n / 2 - 1)
        eps = cc[first + m]
        rep = pair.decide(eps)
        trace.append(rep)
        if rep:
            n = m + 1
        else:
            first, n = first + m + 1, n - (m + 1)
    return eps, trace


def follower_pair(rng, n0, n1):
    """The pair generator of tests/golden/make_golden_traj_dist.py: a base trajectory and a
    noisy re-sampling of it with both end points pinned."""
    t = np.linspace(0.0, 1.0, n0) if n0 > 1 else np.zeros(1)
    base = np.stack([48.0 + 3.0 * t + 0.02 * np.cumsum(rng.standard_normal(n0)),
                     2.0 + 5.0 * t + 0.02 * np.cumsum(rng.standard_normal(n0))], axis=1)
    u = np.sort(rng.uniform(0.0, 1.0, n1))
    u[0], u[-1] = 0.0, 1.0
    k = np.arange(n0, dtype=np.float64)
    fol = np.stack([np.interp(u * (n0 - 1), k, base[:, 0]), np.interp(u * (n0 - 1), k, base[:, 1])],
                   axis=1)
    return base, fol + 0.004 * rng.standard_normal((n1, 2))


def bound(gap, scale):
    return np.maximum(8.0 * gap, 64.0 * U) * scale


# ---- golden access -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def G():
    d = golden("g15_frechet.npz")
    o0, o1 = d["off0"], d["off1"]
    pairs = [(d["pts0"][o0[k]:o0[k + 1]], d["pts1"][o1[k]:o1[k + 1]]) for k in range(len(o0) - 1)]
    to = d["trace_off"]
    traces = [d["trace"][to[k]:to[k + 1]].astype(bool).tolist() for k in range(len(pairs))]
    return dict(pairs=pairs, names=[str(s) for s in d["names"]], ref=d["ref"], host64=d["host64"],
                ext=d["ext"], scale=d["scale"], gap=float(d["gap"]), traces=traces)


@pytest.fixture(scope="module")
def H(G):
    """The float64 host statement on every golden pair, computed once."""
    return [host_frechet(a, b) for a, b in G["pairs"]]


# ---- CPU ---------------------------------------------------------------------------------
def test_golden_covers_the_required_lengths_and_branches(G):
    lens = [(len(a), len(b)) for a, b in G["pairs"]]
    assert lens[:len(LENGTHS)] == LENGTHS
    assert tuple(G["names"][len(LENGTHS):]) == CONSTRUCTED
    by = dict(zip(G["names"], range(len(lens))))
    # 2 * 129 * 256 + 1 = 66049 values: 17 sort tiles of 4096, five merge passes
    assert 2 * 129 * 256 + 1 > 16 * 4096
    assert G["ref"][by["identical"]] == 0.0 and G["scale"][by["identical"]] == 0.0
    # the moved end point is the largest critical value's floor: the search ends on cc[0]
    t0, t1 = G["pairs"][by["end moved"]]
    end_point = max(np.hypot(*(t0[0] - t1[0])), np.hypot(*(t0[-1] - t1[-1])))
    assert abs(G["ref"][by["end moved"]] - end_point) <= 4 * U * end_point
    t0, t1 = G["pairs"][by["repeated points"]]
    assert (np.diff(t0, axis=0) == 0).all(axis=1).sum() >= 2
    assert (np.diff(G["pairs"][by["vertical run in Q"]][1][:, 0]) == 0).sum() >= 2
    assert (np.diff(G["pairs"][by["vertical run in P"]][0][:, 0]) == 0).sum() >= 2
    t0, t1 = G["pairs"][by["float32 values"]]
    assert (t0 == t0.astype(np.float32)).all() and (t1 == t1.astype(np.float32)).all()
    assert (len(t0), len(t1)) == (64, 65)
    # both ways a search can end
    assert any(t and not t[-1] for t in G["traces"]) and any(t and t[-1] for t in G["traces"])
    assert 0 <= G["gap"] < 1e-9


def test_host_statement_matches_the_golden(G, H):
    for k, (value, trace) in enumerate(H):
        lim = bound(G["gap"], G["scale"][k])
        for what in ("ref", "host64", "ext"):
            err = abs(float(value) - G[what][k])
            print(f"{G['names'][k]}: host {float(value):.17g} {what} {G[what][k]:.17g} "
                  f"err {err:.3g} bound {lim:.3g}")
            assert err <= lim, (G["names"][k], what, float(value), G[what][k])
        assert trace == G["traces"][k], G["names"][k]


def test_exports():
    from timevqvae.evaluation import flyability_utils as fu
    from timevqvae.evaluation.flyability_utils import trajectory_distances as td
    assert "frechet_device" in fu.__all__ and callable(fu.frechet_device)
    assert callable(td.frechet) and callable(td.frechet_device)
    assert not hasattr(fu, "frechet") and "frechet" not in fu.__all__
    assert len(fu.COLUMNS) == 13


def test_wrappers_refuse_bad_input():
    from timevqvae.evaluation.flyability_utils import frechet_device
    from timevqvae.evaluation.flyability_utils.trajectory_distances import frechet, max_len
    a, b = np.zeros((3, 2)), np.ones((4, 2))
    with pytest.raises(ValueError, match="2 generated and 1 simulated"):
        frechet_device([a, a], [b])
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        frechet_device([np.zeros((3, 3))], [b])
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        frechet(np.zeros(6), b)
    with pytest.raises(ValueError, match="float32 or float64"):
        frechet_device([a], [np.ones((4, 2), np.int64)])
    with pytest.raises(ValueError, match="at least 1"):
        frechet_device([a], [np.ones((0, 2))])
    with pytest.raises(ValueError, match="limit"):
        frechet(np.zeros((max_len() + 1, 2)), b)
    # 2 * 19 * 29 + 1 values take one 4096-value tile in each half: more than 1000 bytes
    with pytest.raises(ValueError, match="workspace"):
        frechet_device([np.zeros((20, 2))], [np.ones((30, 2))], workspace_bytes=1000)
    with pytest.raises(ValueError, match="pair 1 "):
        frechet_device([a, np.zeros((200, 2))], [b, np.ones((300, 2))], workspace_bytes=1 << 17)


def test_workspace_is_counted_from_the_lengths():
    from timevqvae.hip._native import value
    h0, h1 = np.array([0, 20, 150, 151], np.int64), np.array([0, 30, 287, 292], np.int64)
    per = [int(value("tvq_traj_frechet_workspace", h0[k:].ctypes.data, h1[k:].ctypes.data, 1))
           for k in range(3)]
    vals = [2 * 19 * 29 + 1, 2 * 129 * 256 + 1, 1]
    for got, v in zip(per, vals):
        assert got >= 16 * v and got % 8 == 0
    both = int(value("tvq_traj_frechet_workspace", h0.ctypes.data, h1.ctypes.data, 3))
    assert max(per) < both <= sum(per)
    assert int(value("tvq_traj_frechet_workspace", h0.ctypes.data, h1.ctypes.data, 0)) == 0
    h0[1] = 0  # an empty trajectory is refused
    assert int(value("tvq_traj_frechet_workspace", h0.ctypes.data, h1.ctypes.data, 3)) == -1


# ---- GPU ---------------------------------------------------------------------------------
def _dev(gen, sim, **kw):
    from timevqvae.evaluation.flyability_utils import frechet_device
    return frechet_device(gen, sim, **kw)


@pytest.fixture(scope="module")
def dev_values(G, cuda):
    """The device's values of the golden pairs, one batch."""
    out = _dev([a for a, _ in G["pairs"]], [b for _, b in G["pairs"]], device=cuda)
    assert out.dtype.is_floating_point and out.element_size() == 8 and out.is_cuda
    return out.cpu().numpy()


@pytest.mark.gpu
def test_device_matches_the_reference_on_the_golden_pairs(G, dev_values):
    bad = []
    for k, name in enumerate(G["names"]):
        err, lim = abs(dev_values[k] - G["ref"][k]), bound(G["gap"], G["scale"][k])
        print(f"{name}: device {dev_values[k]:.17g} ref {G['ref'][k]:.17g} err {err:.3g} "
              f"bound {lim:.3g}")
        if not err <= lim:
            bad.append((name, dev_values[k], G["ref"][k], err, lim))
    assert not bad, bad
    assert dev_values[G["names"].index("identical")] == 0.0


@pytest.mark.gpu
def test_device_value_does_not_depend_on_the_batch(G, dev_values, cuda):
    t0s, t1s = [a for a, _ in G["pairs"]], [b for _, b in G["pairs"]]
    for k in range(len(t0s)):
        alone = _dev([t0s[k]], [t1s[k]], device=cuda).cpu().numpy()
        assert alone.shape == (1,) and alone[0] == dev_values[k], G["names"][k]
    perm = np.random.default_rng(0).permutation(len(t0s))
    shuffled = _dev([t0s[k] for k in perm], [t1s[k] for k in perm], device=cuda).cpu().numpy()
    assert np.array_equal(shuffled, dev_values[perm])
    # 3 MiB hold either long pair (2.1 MiB) alone but not both: several chunks
    from timevqvae.evaluation.flyability_utils import trajectory_distances as td
    budget = 3 << 20
    assert len(td._frechet_chunks(td._offsets(t0s), td._offsets(t1s), budget)) > 1
    chunked = _dev(t0s, t1s, device=cuda, workspace_bytes=budget).cpu().numpy()
    assert np.array_equal(chunked, dev_values)


@pytest.mark.gpu
def test_device_float32_inputs(G, dev_values, cuda):
    import torch
    k = G["names"].index("float32 values")
    t0, t1 = G["pairs"][k]
    a32, b32 = t0.astype(np.float32), t1.astype(np.float32)
    assert _dev([a32], [b32], device=cuda).cpu().numpy()[0] == dev_values[k]
    assert _dev([torch.from_numpy(a32)], [torch.from_numpy(b32)],
                device=cuda).cpu().numpy()[0] == dev_values[k]
    assert _dev([torch.from_numpy(a32).to(cuda)], [torch.from_numpy(b32).to(cuda)]
                ).cpu().numpy()[0] == dev_values[k]
    assert _dev([torch.from_numpy(a32).to(cuda)], [t1], device=cuda).cpu().numpy()[0] == dev_values[k]


@pytest.mark.gpu
def test_per_pair_function_and_dict_equal_the_batch(G, dev_values, cuda):
    from timevqvae.evaluation import calculate_trajectory_distances
    from timevqvae.evaluation.flyability_utils import trajectory_distances as td
    k = G["names"].index("float32 values")
    one = td.frechet(*G["pairs"][k])
    assert type(one) is float and one == dev_values[k]
    keep = [k for k, (a, b) in enumerate(G["pairs"]) if min(len(a), len(b)) >= 2]
    t0s, t1s = [G["pairs"][k][0] for k in keep], [G["pairs"][k][1] for k in keep]
    base = calculate_trajectory_distances(t0s, t1s, 47.5, 1.5)
    res = calculate_trajectory_distances(t0s, t1s, 47.5, 1.5, frechet=True)
    assert tuple(res) == KEYS14 and tuple(base) == KEYS14[:13]
    for name in KEYS14[:13]:
        assert res[name] == base[name], name
    assert all(type(v) is float for v in res["Frechet"])
    assert res["Frechet"] == dev_values[keep].tolist()
    assert calculate_trajectory_distances([], [], 0.0, 0.0, frechet=True) == {n: [] for n in KEYS14}


@pytest.mark.gpu
def test_device_long_thin_pair(G, cuda):
    """(1025, 3): 1024 rows of a two-column grid, two full row bands of the decision kernel
    (512 rows of one 64-column word each)."""
    rng = np.random.default_rng(5)
    s = np.linspace(0.0, 1.0, 1025)
    t0 = np.stack([48.0 + 3.0 * s, 2.0 + 5.0 * s], axis=1) + 0.003 * rng.standard_normal((1025, 2))
    t1 = np.array([[48.01, 1.99], [49.4, 4.6], [51.02, 6.97]])
    value, trace = host_frechet(t0, t1)
    dev = _dev([t0], [t1], device=cuda).cpu().numpy()[0]
    err, lim = abs(dev - float(value)), bound(G["gap"], abs(float(value)))
    print(f"1025 x 3: device {dev:.17g} host {float(value):.17g} err {err:.3g} bound {lim:.3g} "
          f"probes {len(trace)}")
    assert len(trace) >= 8 and err <= lim


@pytest.mark.gpu
def test_device_at_the_length_limit(G, cuda):
    """(limit, 2): one column, every row band; (2, limit): one row of 64 words, the carry
    crosses all of them."""
    from timevqvae.evaluation.flyability_utils.trajectory_distances import max_len
    n = max_len()
    rng = np.random.default_rng(6)
    s = np.linspace(0.0, 1.0, n)
    long = np.stack([48.0 + 3.0 * s, 2.0 + 5.0 * s], axis=1) + 0.0002 * rng.standard_normal((n, 2))
    short = np.array([[48.001, 1.999], [51.002, 6.997]])
    dev = _dev([long, short], [short, long], device=cuda).cpu().numpy()
    for k, (t0, t1) in enumerate(((long, short), (short, long))):
        value, trace = host_frechet(t0, t1)
        err, lim = abs(dev[k] - float(value)), bound(G["gap"], abs(float(value)))
        print(f"{len(t0)} x {len(t1)}: device {dev[k]:.17g} host {float(value):.17g} err {err:.3g} "
              f"bound {lim:.3g} probes {len(trace)} passed {sum(trace)}")
        assert len(trace) >= 10 and 0 < sum(trace) < len(trace) and err <= lim


@pytest.mark.gpu
def test_device_matches_the_host_statement_on_random_pairs(G, cuda):
    """24 follower pairs of 2 to 40 points, lengths drawn at random, in one ragged batch."""
    rng = np.random.default_rng(7)
    pairs = [follower_pair(rng, int(rng.integers(2, 41)), int(rng.integers(2, 41)))
             for _ in range(24)]
    dev = _dev([a for a, _ in pairs], [b for _, b in pairs], device=cuda).cpu().numpy()
    for k, (t0, t1) in enumerate(pairs):
        value, trace = host_frechet(t0, t1)
        err, lim = abs(dev[k] - float(value)), bound(G["gap"], abs(float(value)))
        print(f"{len(t0)} x {len(t1)}: device {dev[k]:.17g} host {float(value):.17g} err {err:.3g} "
              f"bound {lim:.3g}")
        assert err <= lim, (k, len(t0), len(t1))


@pytest.mark.gpu
def test_empty_batch(cuda):
    out = _dev([], [], device=cuda)
    assert tuple(out.shape) == (0,) and out.dtype.is_floating_point and out.is_cuda
