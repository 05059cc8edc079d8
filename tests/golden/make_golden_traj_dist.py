"""Generate the G14 golden (the flyability evaluation's trajectory distances) from the
REFERENCE evaluation/flyability_utils/trajectory_distances modules, called as
evaluation/flyability_eval.py:271-351 calls them.

Runs only where the reference checkout exists (the build container).  The reference modules
import each other relatively, and importing flyability_utils itself pulls in `traffic` and
`geopy`, so they are loaded by path under a synthetic package whose __path__ is their
directory.  Only the .npz output is committed:

    tests/golden/g14_traj_dist.npz
      pts0 (sum n0, 2), off0 (P+1), pts1, off1   float64 "follower" pairs, ragged
      g (2)                the ERP gap point
      ref (P, 13)          the reference's values, columns in the order of its results dict
                           without "Frechet"; eps = 0.009, spherical LCSS eps * 1e6, spherical
                           EDR eps; nan in the segment columns of a pair with a 1-point side
      eps_edr_b, ref_edr_b (P)   spherical EDR once more with the threshold 9000
      scale (P, 13)        |ext| per column, the pair's largest great-circle distance for
                           spherical SSPD / Hausdorff; ext = the test file's statement in
                           np.longdouble
      gap (13)             max over the pairs of |ref - ext| / scale (0 for the count columns)
      c_t0 (64, 2), c_t1 (65, 2) float32: the (64, 65) pair cast down; c_out32 = the reference
                           on the float32 arrays, c_out64 = on those values as float64;
                           c_scale (13)

Asserted here: every cell cost is at least 1e-9 (relative) away from each threshold it is
compared with, and every u of point_to_seg at least 1e-9 away from 0.00001 and from 1.

    python tests/golden/make_golden_traj_dist.py
"""
import importlib
import importlib.machinery
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402
from test_traj_dist import (COUNT_COLS, EPS, SPH_SEG_COLS, _eucl, _gcd, host_distances,  # noqa: E402
                            point_to_seg_u, sph_scale)

LENGTHS = [(1, 1), (1, 5), (5, 1), (2, 2), (2, 3), (63, 64), (64, 65), (65, 63), (130, 257),
           (257, 130), (300, 70)]  # the last: 299 segments > the 256-segment tile, 5 row bands
SEED = 14
G = (47.5, 1.5)
EPS_EDR_B = 9000.0
MARGIN = 1e-9


def load_reference():
    d = f"{REF}/evaluation/flyability_utils/trajectory_distances"
    pkg = types.ModuleType("ref_traj_dist")
    pkg.__path__ = [d]
    pkg.__spec__ = importlib.machinery.ModuleSpec("ref_traj_dist", None, is_package=True)
    sys.modules["ref_traj_dist"] = pkg
    ns = types.SimpleNamespace()
    for mod in ("dtw", "erp", "edr", "lcss", "sspd", "hausdorff", "discret_frechet"):
        m = importlib.import_module(f"ref_traj_dist.{mod}")
        for k, v in vars(m).items():
            if callable(v) and (k[:2] in ("e_", "s_") or k == "discret_frechet"):
                setattr(ns, k, v)
    return ns


def follower_pair(rng, n0, n1):
    """A base trajectory and a follower: the base re-sampled at sorted random positions along
    its length (both end points pinned) plus noise."""
    t = np.linspace(0.0, 1.0, n0) if n0 > 1 else np.zeros(1)
    base = np.stack([48.0 + 3.0 * t + 0.02 * np.cumsum(rng.standard_normal(n0)),
                     2.0 + 5.0 * t + 0.02 * np.cumsum(rng.standard_normal(n0))], axis=1)
    u = np.sort(rng.uniform(0.0, 1.0, n1))
    u[0], u[-1] = 0.0, 1.0
    pos = u * (n0 - 1)
    k = np.arange(n0, dtype=np.float64)
    fol = np.stack([np.interp(pos, k, base[:, 0]), np.interp(pos, k, base[:, 1])], axis=1)
    return base, fol + 0.004 * rng.standard_normal((n1, 2))


def reference_row(ref, t0, t1, g, eps=EPS):
    """The 13 values in the order of calculate_trajectory_distances' results dict."""
    seg = min(len(t0), len(t1)) >= 2
    nan = float("nan")
    return np.array([
        ref.e_sspd(t0, t1) if seg else nan, ref.s_sspd(t0, t1) if seg else nan,
        ref.e_dtw(t0, t1), ref.s_dtw(t0, t1),
        ref.e_hausdorff(t0, t1) if seg else nan, ref.s_hausdorff(t0, t1) if seg else nan,
        ref.e_lcss(t0, t1, eps), ref.s_lcss(t0, t1, eps * 1e6),
        ref.e_erp(t0, t1, g), ref.s_erp(t0, t1, g),
        ref.e_edr(t0, t1, eps), ref.s_edr(t0, t1, eps),
        ref.discret_frechet(t0, t1)], dtype=np.float64)


def margins(t0, t1):
    """(Euclidean, spherical, u): the smallest relative distance of a cell cost from a threshold
    it is compared with, and of a point_to_seg u from 0.00001 and 1."""
    E = _eucl(t0[:, None, :], t1[None, :, :])
    S = _gcd(t0[:, None, 0], t0[:, None, 1], t1[None, :, 0], t1[None, :, 1], np.float64)
    me = np.abs(E - EPS).min() / EPS
    ms = min(np.abs(S - th).min() / th for th in (EPS, EPS * 1e6, EPS_EDR_B))
    mu = np.inf
    if min(len(t0), len(t1)) >= 2:
        for A, B in ((t0, t1), (t1, t0)):
            u = point_to_seg_u(A, B)
            u = u[~np.isnan(u)]
            mu = min(mu, np.abs(u - 0.00001).min(), np.abs(u - 1.0).min())
    return me, ms, mu


def scale_of(ext, t0, t1):
    s = np.abs(ext.astype(np.float64))
    s[list(SPH_SEG_COLS)] = sph_scale(t0, t1)
    return s


def main():
    ref = load_reference()
    rng = np.random.default_rng(SEED)
    pairs = [follower_pair(rng, n0, n1) for n0, n1 in LENGTHS]
    g = np.array(G)
    worst = np.array([np.inf, np.inf, np.inf])
    rows, rows_b, scale_rows = [], [], []
    gap = np.zeros(13)
    t_start = time.time()
    for t0, t1 in pairs:
        m = margins(t0, t1)
        assert min(m) >= MARGIN, (t0.shape, t1.shape, m)
        worst = np.minimum(worst, m)
        r = reference_row(ref, t0, t1, g)
        seg = min(len(t0), len(t1)) >= 2
        ext = host_distances(t0, t1, g, T=np.longdouble, segment=seg)
        h64 = host_distances(t0, t1, g, segment=seg)
        sc = scale_of(ext, t0, t1)
        for c in range(13):
            if c in COUNT_COLS:  # the same counts in both precisions
                assert r[c] == h64[c] and abs(r[c] - float(ext[c])) < 1e-15, (c, r[c], ext[c])
            elif not np.isnan(r[c]):
                gap[c] = max(gap[c], float(abs(np.longdouble(r[c]) - ext[c])) / sc[c])
        rows.append(r)
        scale_rows.append(sc)
        rows_b.append(float(ref.s_edr(t0, t1, EPS_EDR_B)))
        assert rows_b[-1] == host_distances(t0, t1, g, eps_edr_s=EPS_EDR_B, segment=False)[11]
        print(f"{len(t0):4d} x {len(t1):4d}: margins {m[0]:.3g} {m[1]:.3g} {m[2]:.3g}  "
              + " ".join(f"{v:.6g}" for v in r), flush=True)
    print(f"reference time for the {len(pairs)} pairs: {time.time() - t_start:.1f} s")
    print("smallest margins (Euclidean, spherical, u):", " ".join(f"{v:.3g}" for v in worst))
    d = {"g": g, "eps_edr_b": np.float64(EPS_EDR_B),
         "pts0": np.concatenate([a for a, _ in pairs]), "pts1": np.concatenate([b for _, b in pairs]),
         "off0": np.concatenate([[0], np.cumsum([len(a) for a, _ in pairs])]).astype(np.int64),
         "off1": np.concatenate([[0], np.cumsum([len(b) for _, b in pairs])]).astype(np.int64),
         "ref": np.stack(rows), "ref_edr_b": np.array(rows_b), "scale": np.stack(scale_rows),
         "gap": gap}

    # the float32 case: the (64, 65) pair cast down, through the reference both ways
    c0, c1 = (a.astype(np.float32) for a in pairs[LENGTHS.index((64, 65))])
    w0, w1 = c0.astype(np.float64), c1.astype(np.float64)
    assert min(margins(w0, w1)) >= MARGIN, margins(w0, w1)
    d["c_t0"], d["c_t1"] = c0, c1
    d["c_out32"] = reference_row(ref, c0, c1, g)
    d["c_out64"] = reference_row(ref, w0, w1, g)
    d["c_scale"] = scale_of(host_distances(w0, w1, g, T=np.longdouble), w0, w1)
    print("float32 case, |ref32 - ref64| / scale:",
          " ".join(f"{v:.3g}" for v in np.abs(d["c_out32"] - d["c_out64"]) / np.maximum(d["c_scale"], 1e-300)))
    print("gap:", " ".join(f"{v:.3g}" for v in gap))
    for k in ("ref", "c_out32", "c_out64"):
        assert np.isfinite(d[k][~np.isnan(d[k])]).all(), k

    # the reference's host time for one pair of the timing tool's size (13 distances)
    t0, t1 = follower_pair(np.random.default_rng(SEED + 1), 200, 300)
    t_start = time.time()
    reference_row(ref, t0, t1, g)
    print(f"reference host time, one 200 x 300 pair, 13 distances: {time.time() - t_start:.2f} s")

    path = os.path.join(HERE, "g14_traj_dist.npz")
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(f"wrote g14_traj_dist.npz: {size} bytes")


if __name__ == "__main__":
    main()
