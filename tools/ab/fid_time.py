"""fid_device (csrc/tvq_fid.hip) alone with device events: the "few" form at (N1, N2, D) =
(1000, 900, 2000) with max_sweeps 16 and the "many" form at (3000, 2500, 128), the shapes of
profiles/fid_device.txt.  Inputs: L2-normalised Gaussian features, the second set scaled 1.3 and
shifted 0.2, resident on the device.  Median, min and max of --runs calls after two warm-ups.
Uses the package's public functions only, so --root TREE times another checkout's build.

usage: python tools/ab/fid_time.py [--root TREE] [--runs 20]"""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser(usage=__doc__)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__)))))
ap.add_argument("--runs", type=int, default=20)
args = ap.parse_args()
sys.path.insert(0, os.path.join(args.root, "t-vq-vae-trajgen_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from timevqvae.evaluation import fid_device  # noqa: E402


def feats(rng, n, d, scale=1.0, shift=0.0):
    z = rng.standard_normal((n, d))
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    return torch.from_numpy(scale * z + shift).cuda()


for name, (n1, n2, d), kw in (("few", (1000, 900, 2000), {"max_sweeps": 16}),
                              ("many", (3000, 2500, 128), {})):
    rng = np.random.default_rng(5)
    z1, z2 = feats(rng, n1, d), feats(rng, n2, d, 1.3, 0.2)
    for _ in range(2):
        v = fid_device(z1, z2, **kw)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        v = fid_device(z1, z2, **kw)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    print(f"fid {name} ({n1}, {n2}, {d}) value {float(v)!r}: median {statistics.median(ts):.3f} ms "
          f"(min {min(ts):.3f}, max {max(ts):.3f}), {args.runs} runs", flush=True)
