"""The supervised FCN extractor's features (timevqvae.evaluation.fcn_features, csrc/tvq_fcn.hip)
for an evaluation set of 8192 samples of (6, 256) in batches of 256, against the same network
in torch eager eval on the same GPU.

After a warm-up, `--runs` times (at least 21) and alternating in one process: `fcn_features`
end to end from the host array (upload, three conv launches, download per batch) and the
eager statement of the same loop (F.pad + F.conv1d, F.batch_norm eval, relu, mean), each
between device events; then each of the three conv launches alone on one resident batch, and
the three eager blocks likewise.  Medians are reported.  FLOPs are counted from the shapes
(2 L (Ci 8 128 + 128 5 256 + 256 3 128) per sample) and set against the 155 TF fp32 MFMA peak.

Writes one JSON (default profiles/fcn_time.json) and prints it.  Needs a GPU.

usage: python tools/fcn_time.py [--runs 21] [--n 8192] [--channels 6] [--length 256]
                                [--batch 256] [--out F]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "t-vq-vae-trajgen_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=21)
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--channels", type=int, default=6)
ap.add_argument("--length", type=int, default=256)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fcn_time.json"))
args = ap.parse_args()
if args.runs < 21:
    sys.exit("fcn_time: at least 21 runs")

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from timevqvae.evaluation import fcn_features  # noqa: E402
from timevqvae.evaluation.metrics import batched  # noqa: E402
from timevqvae.hip import fcn as ops  # noqa: E402
from timevqvae.models import FCNBaseline  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("fcn_time: no GPU (the device path has no CPU fallback)")
dev = torch.device("cuda:0")
PEAK_TF = 155.0

torch.manual_seed(17)
fcn = FCNBaseline(args.channels, 5)
with torch.no_grad():  # non-trivial BatchNorm statistics
    for blk in fcn.layers:
        bn = blk.layers[1]
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.5, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
fcn = fcn.to(dev).eval()
rng = np.random.default_rng(17)
X = np.cumsum(0.1 * rng.standard_normal((args.n, args.channels, args.length)), -1).astype(np.float32)


def eager_block(h, i):
    conv, bn = fcn.layers[i].layers[0], fcn.layers[i].layers[1]
    K = conv.weight.shape[2]
    h = F.conv1d(F.pad(h, ((K - 1) // 2, K - 1 - (K - 1) // 2)), conv.weight, conv.bias)
    return F.relu(F.batch_norm(h, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0,
                               bn.eps))


@torch.no_grad()
def eager_features(x):
    def one(xb):
        h = torch.from_numpy(xb).to(dev)
        for i in range(3):
            h = eager_block(h, i)
        return h.mean(-1).cpu().numpy()
    return batched(one, x, args.batch)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def alternate(fa, fb):
    ta, tb = [], []
    for _ in range(args.runs):
        ta.append(timed(fa))
        tb.append(timed(fb))
    return stats(ta), stats(tb)


# warm-up of both paths, and the two must agree
zh, ze = fcn_features(fcn, X, args.batch), eager_features(X)
err = float(np.abs(zh - ze).max() / np.abs(ze).max())
assert err <= 2e-5, err
res = {"n": args.n, "channels": args.channels, "length": args.length, "batch": args.batch,
       "runs": args.runs, "device": torch.cuda.get_device_name(0), "peak_tf_fp32_mfma": PEAK_TF,
       "hip_vs_eager_max_err_over_max": err, "ms": {}}
res["ms"]["hip_end_to_end"], res["ms"]["eager_end_to_end"] = alternate(
    lambda: fcn_features(fcn, X, args.batch), lambda: eager_features(X))

# the three launches on one resident batch
xb = torch.from_numpy(X[:args.batch]).to(dev)
acts, layers = [xb], [ops._layer(fcn, i) for i in range(3)]
for i in range(2):
    acts.append(ops.conv_bn_relu(acts[i], *layers[i][:1], *layers[i][2:], packed=layers[i][1])[0])
macs = [args.channels * 8 * 128, 128 * 5 * 256, 256 * 3 * 128]
with torch.no_grad():
    for i in range(3):
        w, wp, scale, shift = layers[i]
        last = i == 2
        hip, eager = alternate(
            lambda: ops.conv_bn_relu(acts[i], w, scale, shift, y=not last, gap=last, packed=wp),
            (lambda: eager_block(acts[i], i).mean(-1)) if last else (lambda: eager_block(acts[i], i)))
        res["ms"][f"hip_conv{i + 1}"], res["ms"][f"eager_block{i + 1}"] = hip, eager
        fl = 2.0 * macs[i] * args.length * args.batch
        res.setdefault("tflops", {})[f"hip_conv{i + 1}"] = fl / (hip["median"] * 1e-3) / 1e12

flops = 2.0 * sum(macs) * args.length * args.n
res["flops"] = flops
for k in ("hip_end_to_end", "eager_end_to_end"):
    res["tflops"][k] = flops / (res["ms"][k]["median"] * 1e-3) / 1e12
launches = sum(res["ms"][f"hip_conv{i}"]["median"] for i in (1, 2, 3))
res["tflops"]["hip_three_launches"] = (2.0 * sum(macs) * args.length * args.batch
                                       / (launches * 1e-3) / 1e12)
res["share_of_peak"] = {k: v / PEAK_TF for k, v in res["tflops"].items()}
res["eager_over_hip_end_to_end"] = (res["ms"]["eager_end_to_end"]["median"]
                                    / res["ms"]["hip_end_to_end"]["median"])
for k, v in res["ms"].items():
    print(f"{k:20s} median {v['median']:9.3f} ms  (min {v['min']:.3f}, max {v['max']:.3f})", flush=True)
for k, v in res["tflops"].items():
    print(f"{k:20s} {v:8.2f} TF = {100 * v / PEAK_TF:5.1f} % of {PEAK_TF:.0f} TF", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
