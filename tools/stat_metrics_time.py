"""The TSGBench statistics (MDD / ACD / SD / KD) at the notebook's real shapes -- real
(660, 4, 4633) against generated (1024, 4, 4633), float32 synthetic random walks -- on the
device (timevqvae.evaluation.stat_metrics, csrc/tvq_stat.hip) and the same formulas in numpy on
the host's permitted cores.

Device: after a warm-up, each kernel group (moments, KDE, ACF; both sets) is timed with
device events around the launches, `--runs` times, median reported; `stat_metrics_device`
from host float32 arrays (upload, the three groups, the read-backs) is timed with a host
clock around a synchronise.  Work is counted from the shapes: one exp per (sample, grid
point), N L (L + 1) / 2 FMA per set; shares are of the fp64 vector peak (78.6 TFLOP/s spec =
39.3e12 FMA/s).  Host: the KDE in chunks and np.correlate per series over a pool of
`--threads` threads (numpy releases the GIL), run once (about a minute).  Agreement is held
at the bounds of tests/test_stat_metrics.py.  Prints one JSON line at the end.

usage: python tools/stat_metrics_time.py [--runs 7] [--threads 16] [--scale 1.0] [--no-host]"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "t-vq-vae-trajgen_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
ap.add_argument("--scale", type=float, default=1.0, help="fraction of the series (rehearsal)")
ap.add_argument("--no-host", action="store_true")
args = ap.parse_args()

FP64_FMA_PEAK = 39.3e12
U = 2.0 ** -53
C, L, G = 4, 4633, 100
N_REAL, N_GEN = max(2, int(660 * args.scale)), max(2, int(1024 * args.scale))
rng = np.random.default_rng(0)
real = (np.cumsum(rng.standard_normal((N_REAL, C, L)), -1) * 0.1).astype(np.float32)
gen = (0.2 + np.cumsum(rng.standard_normal((N_GEN, C, L)), -1) * 0.1).astype(np.float32)


# ---- host: the same formulas in float64 numpy ------------------------------------------------
def host_moments(x):
    mean = x.sum() / x.size
    d = x - mean
    d2 = d * d
    return mean, d2.sum() / x.size, (d2 * d).sum() / x.size, (d2 * d2).sum() / x.size


def host_kde(pool, x, grid):
    s = np.std(x, ddof=1) * x.size ** (-0.2)
    xs, gs = x / s, grid / s

    def part(chunk):
        return np.array([np.exp(-0.5 * (g - chunk) ** 2).sum() for g in gs])
    parts = list(pool.map(part, np.array_split(xs, 16 * args.threads)))
    return np.sum(parts, axis=0) / (x.size * s * np.sqrt(2.0 * np.pi))


def host_acf(pool, x):
    rows = x[:, 0, :]
    return np.mean(list(pool.map(lambda r: np.correlate(r, r, mode="full")[L - 1:], rows)), axis=0)


def host_all():
    out, t = {}, {}
    r64, g64 = real.astype(np.float64), gen.astype(np.float64)
    with ThreadPoolExecutor(args.threads) as pool:
        t0 = time.perf_counter()
        mr, mg = host_moments(r64.reshape(-1)), host_moments(g64.reshape(-1))
        out["sd"] = abs(mr[2] / mr[1] ** 1.5 - mg[2] / mg[1] ** 1.5)
        out["kd"] = abs(mr[3] / mr[1] ** 2 - mg[3] / mg[1] ** 2)
        t["moments"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        grid = np.linspace(float(min(r64.min(), g64.min())), float(max(r64.max(), g64.max())), G)
        dr, dg = host_kde(pool, r64.reshape(-1), grid), host_kde(pool, g64.reshape(-1), grid)
        out["mdd"] = np.mean(np.abs(dr - dg))
        t["kde"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        ar, ag = host_acf(pool, r64), host_acf(pool, g64)
        out["acd"] = np.mean(np.abs(ar - ag))
        t["acf"] = time.perf_counter() - t0
    bounds = {"mdd": 1e-10 * 0.5 * (dr.mean() + dg.mean()), "acd": 4 * L * U * (ar[0] + ag[0]),
              "sd": 2.5e-10 * (abs(mr[2] / mr[1] ** 1.5) + abs(mg[2] / mg[1] ** 1.5)),
              "kd": 3e-10 * (mr[3] / mr[1] ** 2 + mg[3] / mg[1] ** 2)}
    return out, t, bounds


# ---- device ------------------------------------------------------------------------------------
import torch  # noqa: E402

from timevqvae.evaluation import stat_metrics as sm  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("stat_metrics_time: no GPU (the device path has no CPU fallback)")
dev = torch.device("cuda:0")


def median_ms(fn, sync_clock=False):
    ts = []
    for _ in range(args.runs):
        if sync_clock:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


xr, xg = sm._upload(real, dev)[0], sm._upload(gen, dev)[0]
full = sm.stat_metrics_device(real, gen, dev)  # warm-up of every kernel at these shapes
grid = full.grid
sr = sm.scott_bandwidth(xr.numel(), float(full.moments_real[3]))
sg = sm.scott_bandwidth(xg.numel(), float(full.moments_gen[3]))
res = {"shapes": {"real": list(real.shape), "gen": list(gen.shape), "grid": G}, "device_ms": {}}
groups = {
    "moments": lambda: (sm.moments_device(xr), sm.moments_device(xg)),
    "kde": lambda: (sm.kde_device(xr.reshape(-1), grid, sr), sm.kde_device(xg.reshape(-1), grid, sg)),
    "acf": lambda: (sm.acf_mean_device(xr), sm.acf_mean_device(xg)),
}
for name, fn in groups.items():
    fn()
    med, lo, hi = median_ms(fn)
    res["device_ms"][name] = {"median": med, "min": lo, "max": hi}
    print(f"device {name:8s} median {med:9.3f} ms  (min {lo:.3f}, max {hi:.3f}, {args.runs} runs)",
          flush=True)
med, lo, hi = median_ms(lambda: sm.stat_metrics_device(real, gen, dev), sync_clock=True)
res["device_ms"]["end_to_end_from_host_float32"] = {"median": med, "min": lo, "max": hi}
print(f"device end to end (upload + all four) median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})",
      flush=True)
n_exp = (xr.numel() + xg.numel()) * G
n_fma = (N_REAL + N_GEN) * L * (L + 1) // 2
n_bytes = 2 * 8 * (xr.numel() + xg.numel())  # two passes over float64
res["work"] = {"kde_exp": n_exp, "acf_fma": n_fma, "moments_bytes": n_bytes}
res["rates"] = {
    "kde_exp_per_s": n_exp / (res["device_ms"]["kde"]["median"] * 1e-3),
    "acf_fma_per_s": n_fma / (res["device_ms"]["acf"]["median"] * 1e-3),
    "acf_share_of_fp64_fma_peak": n_fma / (res["device_ms"]["acf"]["median"] * 1e-3) / FP64_FMA_PEAK,
    "moments_bytes_per_s": n_bytes / (res["device_ms"]["moments"]["median"] * 1e-3),
}
for k, v in res["rates"].items():
    print(f"{k}: {v:.4g}", flush=True)
res["device"] = dict(zip(("mdd", "acd", "sd", "kd"), full[:4]))

if not args.no_host:
    host, t, bounds = host_all()
    res["host_s"], res["host"] = t, {k: float(v) for k, v in host.items()}
    res["host_threads"] = args.threads
    res["agreement"] = {}
    for k in ("mdd", "acd", "sd", "kd"):
        err = abs(res["device"][k] - host[k])
        res["agreement"][k] = {"abs_err": float(err), "bound": float(bounds[k]),
                               "ok": bool(err <= bounds[k])}
        print(f"{k}: device {res['device'][k]:.15g} host {host[k]:.15g} |err| {err:.3g} "
              f"bound {bounds[k]:.3g} {'ok' if err <= bounds[k] else 'MISS'}", flush=True)
    for k, v in t.items():
        print(f"host {k:8s} {v:8.2f} s on {args.threads} threads", flush=True)
print(json.dumps(res))
