"""The flyability evaluation's trajectory distances for a batch of 1024 "follower" pairs of
200 x 300 points (float64, the generator of tests/golden/make_golden_traj_dist.py) on the device
(timevqvae.evaluation.flyability_utils, csrc/tvq_traj.hip).

After a warm-up each kernel family (table: DTW / ERP / EDR / LCSS / discrete Frechet; segment:
SSPD / Hausdorff) is timed with device events around its one launch on the packed batch,
`--runs` times (at least 20), median reported; the upload (packing on the host, one copy,
widening on the device) and `trajectory_distances_device` end to end from the host arrays are
timed with a host clock around a synchronise.  Cell rates are counted from the shapes
(n0 n1 cells per pair and geometry; n0 (n1 - 1) + n1 (n0 - 1) point-segment pairs).

The continuous Frechet distance (csrc/tvq_traj_frechet.hip) is a leg of its own on the same
pairs: `tvq_traj_frechet` on the packed batch with one workspace for all pairs, and its stages
through `tvq_traj_frechet_stages` (critical values; critical values + sort and unique, whose
difference is the sort's share; the search on what those left), device events, the same
median.  Written under the key "frechet" with the probe count from the value count.

Writes one JSON (default profiles/traj_dist_time.json) and prints it.

usage: python tools/traj_dist_time.py [--runs 21] [--pairs 1024] [--n0 200] [--n1 300] [--out F]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "t-vq-vae-trajgen_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=21)
ap.add_argument("--pairs", type=int, default=1024)
ap.add_argument("--n0", type=int, default=200)
ap.add_argument("--n1", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_dist_time.json"))
args = ap.parse_args()
if args.runs < 20:
    sys.exit("traj_dist_time: at least 20 runs")

import torch  # noqa: E402

from timevqvae.evaluation.flyability_utils import trajectory_distances as td  # noqa: E402
from timevqvae.hip._native import call, ptr, stream_ptr  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("traj_dist_time: no GPU (the device path has no CPU fallback)")
dev = torch.device("cuda:0")
EPS, G = 0.009, (47.5, 1.5)


def follower_pair(rng, n0, n1):
    t = np.linspace(0.0, 1.0, n0)
    base = np.stack([48.0 + 3.0 * t + 0.02 * np.cumsum(rng.standard_normal(n0)),
                     2.0 + 5.0 * t + 0.02 * np.cumsum(rng.standard_normal(n0))], axis=1)
    u = np.sort(rng.uniform(0.0, 1.0, n1))
    u[0], u[-1] = 0.0, 1.0
    k = np.arange(n0, dtype=np.float64)
    fol = np.stack([np.interp(u * (n0 - 1), k, base[:, 0]), np.interp(u * (n0 - 1), k, base[:, 1])],
                   axis=1)
    return base, fol + 0.004 * rng.standard_normal((n1, 2))


rng = np.random.default_rng(15)
pairs = [follower_pair(rng, args.n0, args.n1) for _ in range(args.pairs)]
gen, sim = [a for a, _ in pairs], [b for _, b in pairs]
P = len(pairs)


def median_ms(fn, events):
    ts = []
    for _ in range(args.runs):
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        else:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


t0s = [torch.from_numpy(a) for a in gen]
t1s = [torch.from_numpy(b) for b in sim]
pts0, off0, pts1, off1, h0, h1 = td._pack(t0s, t1s, dev)
out = torch.zeros(P, 13, dtype=torch.float64, device=dev)


def table():
    call("tvq_traj_table_distances", ptr(pts0), ptr(off0), ptr(pts1), ptr(off1), h0.ctypes.data,
         h1.ctypes.data, P, G[0], G[1], EPS, EPS * 1e6, EPS, ptr(out), stream_ptr())


def segment():
    call("tvq_traj_segment_distances", ptr(pts0), ptr(off0), ptr(pts1), ptr(off1), h0.ctypes.data,
         h1.ctypes.data, P, ptr(out), stream_ptr())


full = td.trajectory_distances_device(gen, sim, G, device=dev)  # warm-up of everything
table()
segment()
torch.cuda.synchronize()
assert torch.equal(out, full)
res = {"pairs": P, "n0": args.n0, "n1": args.n1, "runs": args.runs,
       "device": torch.cuda.get_device_name(0), "ms": {}}
res["ms"]["table"] = median_ms(table, True)
res["ms"]["segment"] = median_ms(segment, True)
res["ms"]["upload"] = median_ms(lambda: td._pack(t0s, t1s, dev), False)
res["ms"]["end_to_end_from_host_float64"] = median_ms(
    lambda: td.trajectory_distances_device(gen, sim, G, device=dev), False)
cells = P * args.n0 * args.n1
segs = P * (args.n0 * (args.n1 - 1) + args.n1 * (args.n0 - 1))
res["rates"] = {"table_cells_per_s_per_geometry": cells / (res["ms"]["table"]["median"] * 1e-3),
                "segment_point_segment_pairs_per_s": segs / (res["ms"]["segment"]["median"] * 1e-3)}
res["ms_per_pair_kernels"] = (res["ms"]["table"]["median"] + res["ms"]["segment"]["median"]) / P
res["column_means"] = dict(zip(td.COLUMNS, full.mean(0).tolist()))

# ---- the continuous Frechet distance ------------------------------------------------------
need = td._frechet_bytes(h0, h1, 0, P)
ws = torch.empty(need, dtype=torch.uint8, device=dev)
fout = torch.zeros(P, dtype=torch.float64, device=dev)


def frechet_stages(mask):
    call("tvq_traj_frechet_stages", ptr(pts0), ptr(off0), ptr(pts1), ptr(off1), h0.ctypes.data,
         h1.ctypes.data, P, ptr(fout), ptr(ws), need, mask, stream_ptr())


def frechet_whole():
    call("tvq_traj_frechet", ptr(pts0), ptr(off0), ptr(pts1), ptr(off1), h0.ctypes.data,
         h1.ctypes.data, P, ptr(fout), ptr(ws), need, stream_ptr())


frechet_whole()
torch.cuda.synchronize()
assert torch.equal(fout, td.frechet_device(gen, sim, device=dev, workspace_bytes=need))
fr = {"workspace_bytes": need, "values_per_pair": 2 * (args.n0 - 1) * (args.n1 - 1) + 1, "ms": {}}
fr["ms"]["whole"] = median_ms(frechet_whole, True)
fr["ms"]["stage1_critical_values"] = median_ms(lambda: frechet_stages(1), True)
fr["ms"]["stage1_and_2"] = median_ms(lambda: frechet_stages(3), True)
fr["ms"]["stage3_search"] = median_ms(lambda: frechet_stages(4), True)
fr["ms"]["end_to_end_from_host_float64"] = median_ms(
    lambda: td.frechet_device(gen, sim, device=dev, workspace_bytes=need), False)
fr["ms_stage2_sort_unique"] = (fr["ms"]["stage1_and_2"]["median"]
                               - fr["ms"]["stage1_critical_values"]["median"])
fr["ms_per_pair"] = fr["ms"]["whole"]["median"] / P
fr["mean"] = float(fout.mean())
res["frechet"] = fr
for k, v in fr["ms"].items():
    print(f"frechet {k:24s} median {v['median']:9.3f} ms  (min {v['min']:.3f}, max {v['max']:.3f})",
          flush=True)
for k, v in res["ms"].items():
    print(f"{k:32s} median {v['median']:9.3f} ms  (min {v['min']:.3f}, max {v['max']:.3f})", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
