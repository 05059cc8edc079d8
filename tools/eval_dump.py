"""Every result of the float64 evaluation kernels (csrc/tvq_stat.hip, tvq_traj.hip,
tvq_traj_frechet.hip, tvq_fid.hip, tvq_rocket.hip) as .npy files, for a byte-for-byte comparison
of two builds.  Inputs are the committed goldens (g7, g10, g13 - g16, read from this checkout)
and seeded generators, all finite.  Cases:

  stat     moments_device at n = 2, 255, 256, 257, 100003; kde_device at n in {2, 257, 70001} x
           G in {1, 100, 101}; acf_mean_device at the ACF_SHAPES of tests/test_stat_metrics.py;
           stat_metrics_device on g13 a, b and the float32 case c
  traj     trajectory_distances_device on the g14 pairs: the table family on all of them and
           both families on those of two points or more, each as one batch and pair by pair;
           the table family with the second spherical EDR threshold; the segment family alone;
           seeded pairs of (2, 2), (256, 257) and (257, 513) points (the 256-thread and
           256-segment tile edges of the segment kernel)
  frechet  frechet_device on the g15 pairs as one batch and pair by pair, both again with a
           workspace that forces three chunks or more; a 129 x 130 pair (several sort tiles:
           a merge pass)
  fid      feature_moments on g10 a, b, c and at (1100, 2000); fid_device(return_parts=True) on
           every g16 case, few_a and many_a with either form forced, and (300, 257, 513);
           jacobi_sv at (1, 7), (2, 3), (5, 4), (33, 47), (64, 64) and in stacked mode
  rocket   apply_kernels on g7 a and b

Uses the package's public functions only, so --root TREE dumps another checkout's build.

usage: python tools/eval_dump.py [--root TREE] OUT_DIR    then: diff -r OUT_DIR_A OUT_DIR_B"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser(usage=__doc__)
ap.add_argument("--root", default=HERE)
ap.add_argument("out")
args = ap.parse_args()
sys.path.insert(0, os.path.join(args.root, "t-vq-vae-trajgen_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from timevqvae.evaluation import (apply_kernels, feature_moments, fid_device,  # noqa: E402
                                  stat_metrics_device)
from timevqvae.evaluation.flyability_utils import (frechet_device,  # noqa: E402
                                                   trajectory_distances_device)
from timevqvae.evaluation.stat_metrics import (acf_mean_device, kde_device,  # noqa: E402
                                               moments_device, scott_bandwidth)
from timevqvae.hip.linalg import jacobi_sv  # noqa: E402

ACF_SHAPES = [(1, 1, 1), (3, 2, 2), (5, 3, 63), (5, 3, 64), (7, 4, 65), (130, 1, 255), (4, 2, 1000),
              (3, 2, 2500), (2, 1, 8192)]
OUT = args.out


def golden(name):
    return np.load(os.path.join(HERE, "tests", "golden", name), allow_pickle=False)


def put(name, t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    np.save(os.path.join(OUT, name + ".npy"), a)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def walks(rng, shape, offset=0.0):
    return offset + np.cumsum(rng.standard_normal(shape), axis=-1) * 0.1


def ragged(d):
    o0, o1 = d["off0"], d["off1"]
    return ([d["pts0"][o0[p]:o0[p + 1]] for p in range(len(o0) - 1)],
            [d["pts1"][o1[p]:o1[p + 1]] for p in range(len(o1) - 1)])


def stat():
    for n in (2, 255, 256, 257, 100003):
        x = 3.0 + 0.5 * np.random.default_rng(n).standard_normal(n)
        put(f"stat_moments_n{n}", moments_device(dev(x)))
    for n in (2, 257, 70001):
        for G in (1, 100, 101):
            x = 0.3 + 0.7 * np.random.default_rng(n + G).standard_normal(n)
            xt = dev(x)
            s = scott_bandwidth(n, float(moments_device(xt)[3]))
            put(f"stat_kde_n{n}_G{G}", kde_device(xt, dev(np.linspace(x.min(), x.max(), G)), s))
    for shape in ACF_SHAPES:
        x = walks(np.random.default_rng(sum(shape)), shape, 0.1)
        put("stat_acf_" + "x".join(map(str, shape)), acf_mean_device(dev(x)))
    g = golden("g13_stat.npz")
    for k in "abc":
        r = stat_metrics_device(g[f"{k}_real"], g[f"{k}_gen"])
        for name, v in zip(r._fields, r):
            put(f"stat_g13_{k}_{name}", v)


def traj():
    d = golden("g14_traj_dist.npz")
    t0s, t1s = ragged(d)
    g = tuple(d["g"])
    seg = [p for p in range(len(t0s)) if min(len(t0s[p]), len(t1s[p])) >= 2]
    s0, s1 = [t0s[p] for p in seg], [t1s[p] for p in seg]
    put("traj_g14_table", trajectory_distances_device(t0s, t1s, g, families=("table",)))
    put("traj_g14_table_edr_b", trajectory_distances_device(
        t0s, t1s, g, edr_spherical_eps=float(d["eps_edr_b"]), families=("table",)))
    put("traj_g14_both", trajectory_distances_device(s0, s1, g))
    put("traj_g14_segment", trajectory_distances_device(s0, s1, g, families=("segment",)))
    for p in range(len(t0s)):
        put(f"traj_g14_table_pair{p}",
            trajectory_distances_device([t0s[p]], [t1s[p]], g, families=("table",)))
    for p in seg:
        put(f"traj_g14_both_pair{p}", trajectory_distances_device([t0s[p]], [t1s[p]], g))
    for n0, n1 in ((2, 2), (256, 257), (257, 513)):
        rng = np.random.default_rng(1000 * n0 + n1)
        a = np.array([2.0, 48.0]) + walks(rng, (2, n0), 0.0).T * 0.05
        b = np.array([2.0, 48.0]) + walks(rng, (2, n1), 0.0).T * 0.05
        put(f"traj_seeded_{n0}x{n1}", trajectory_distances_device([a], [b], (2.0, 48.0)))


def frechet():
    d = golden("g15_frechet.npz")
    t0s, t1s = ragged(d)
    # what the largest pair needs alone (two halves of 8-byte values in whole 4096-value sort
    # tiles, after a 256-byte head): the g15 batch then runs in four chunks
    budget = max(256 + 16 * 4096 * -(-(2 * (len(a) - 1) * (len(b) - 1) + 1) // 4096)
                 for a, b in zip(t0s, t1s))
    for tag, kw in (("", {}), ("_chunked", {"workspace_bytes": budget})):
        put(f"frechet_g15_batch{tag}", frechet_device(t0s, t1s, **kw))
        for p in range(len(t0s)):
            put(f"frechet_g15_pair{p}{tag}", frechet_device([t0s[p]], [t1s[p]], **kw))
    rng = np.random.default_rng(129130)
    a, b = walks(rng, (2, 129), 0.0).T, walks(rng, (2, 130), 0.3).T
    put("frechet_seeded_129x130", frechet_device([a], [b]))


def fid():
    g = golden("g10_fid.npz")
    for k in "abc":
        for i in (1, 2):
            mu, sigma = feature_moments(g[f"{k}_z{i}"])
            put(f"fid_g10_{k}_mu{i}", mu)
            put(f"fid_g10_{k}_sigma{i}", sigma)
    mu, sigma = feature_moments(dev(np.random.default_rng(1).standard_normal((1100, 2000))))
    put("fid_moments_1100x2000_mu", mu)
    put("fid_moments_1100x2000_sigma", sigma)

    def whole(tag, z1, z2, **kw):
        _, out, info = fid_device(z1, z2, return_parts=True, **kw)
        put(f"fid_{tag}_out", out)
        put(f"fid_{tag}_info", info)

    g = golden("g16_fid_device.npz")
    for k in (str(s) for s in g["names"]):
        whole(f"g16_{k}", g[f"{k}_z1"], g[f"{k}_z2"])
    for k in ("few_a", "many_a"):
        for form in ("few", "many"):
            whole(f"g16_{k}_forced_{form}", g[f"{k}_z1"], g[f"{k}_z2"], form=form)
    rng = np.random.default_rng(25)
    whole("tile_edge", rng.standard_normal((300, 513)), 1.3 * rng.standard_normal((257, 513)) + 0.2)
    for n, m in ((1, 7), (2, 3), (5, 4), (33, 47), (64, 64)):
        a = dev(np.random.default_rng(100 * n + m).standard_normal((n, m)))
        sigma, info = jacobi_sv(a)
        for name, v in (("sigma", sigma), ("info", info), ("rot", a)):
            put(f"fid_jacobi_{n}x{m}_{name}", v)
    b = np.random.default_rng(22).standard_normal((48, 60))
    s = b @ b.T / 60
    a = dev(np.concatenate([(s + s.T) / 2, np.eye(48)], 1))
    sigma, info = jacobi_sv(a, m_dot=48)
    for name, v in (("sigma", sigma), ("info", info), ("rot", a)):
        put(f"fid_jacobi_stacked_{name}", v)


def rocket():
    g = golden("g7_rocket.npz")
    for tag in "ab":
        k = tuple(g[f"{tag}_{n}"] for n in ("weights", "lengths", "biases", "dilations", "paddings"))
        put(f"rocket_g7_{tag}", apply_kernels(g[f"{tag}_X"], k))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    for family in (stat, traj, frechet, fid, rocket):
        family()
        torch.cuda.synchronize()
        print(f"eval_dump: {family.__name__} done", flush=True)
    print(f"eval_dump: {len(os.listdir(OUT))} files in {OUT}")
