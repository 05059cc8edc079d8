"""One training step of the supervised FCN (trainers.ExpFCN's loop body: zero_grad,
FCNBaseline.loss, backward, FusedAdamW.step; csrc/tvq_fcn_train.hip) at B = 256 samples of
(6, 256), 5 classes, against the torch-eager statement of the same step on the same GPU
(F.pad + F.conv1d, training F.batch_norm, relu, mean, linear, cross_entropy, autograd,
torch.optim.AdamW).

After a warm-up, `--runs` times (at least 21) and alternating in one process, each between
device events; then every launch of the HIP step alone on resident tensors against its eager
counterpart (the wrappers of hip.fcn_train, output allocation included, on both sides).
Medians are reported.  FLOPs are counted from the shapes -- per layer 2 B L Ci K Co for the
forward and for the weight gradient, and for the data gradient of layers 2 and 3 -- and set
against the 155 TF fp32 MFMA peak.

Writes one JSON (default profiles/fcn_train_time.json) and prints it.  Needs a GPU.

usage: python tools/fcn_train_time.py [--runs 21] [--channels 6] [--length 256] [--batch 256]
                                      [--out F]"""
import argparse
import copy
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "t-vq-vae-trajgen_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=21)
ap.add_argument("--channels", type=int, default=6)
ap.add_argument("--length", type=int, default=256)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--classes", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fcn_train_time.json"))
args = ap.parse_args()
if args.runs < 21:
    sys.exit("fcn_train_time: at least 21 runs")

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from timevqvae.hip import fcn_train as ft  # noqa: E402
from timevqvae.hip.optim import FusedAdamW  # noqa: E402
from timevqvae.models import FCNBaseline  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("fcn_train_time: no GPU (the device path has no CPU fallback)")
dev = torch.device("cuda:0")
PEAK_TF = 155.0
B, C, L = args.batch, args.channels, args.length

torch.manual_seed(17)
fcn = FCNBaseline(C, args.classes).to(dev).train()
ref = copy.deepcopy(fcn)  # the eager statement reads the same parameters through plain torch
rng = np.random.default_rng(17)
x = torch.from_numpy(np.cumsum(0.1 * rng.standard_normal((B, C, L)), -1).astype(np.float32)).to(dev)
y = torch.from_numpy(rng.integers(0, args.classes, B)).to(dev)


def pad_same(h, K):
    return F.pad(h, ((K - 1) // 2, K - 1 - (K - 1) // 2))


def eager_loss(m, xb, yb):
    h = xb
    for blk in m.layers:
        conv, bn = blk.layers[0], blk.layers[1]
        h = F.conv1d(pad_same(h, conv.weight.shape[2]), conv.weight, conv.bias)
        h = F.relu(F.batch_norm(h, bn.running_mean, bn.running_var, bn.weight, bn.bias, True,
                                bn.momentum, bn.eps))
    return F.cross_entropy(F.linear(h.mean(-1), m.final.weight, m.final.bias), yb)


opt_h = FusedAdamW(fcn.parameters(), lr=1e-3, weight_decay=1e-5)
opt_e = torch.optim.AdamW(ref.parameters(), lr=1e-3, weight_decay=1e-5)


def hip_step():
    opt_h.zero_grad()
    loss, _ = fcn.loss(x, y)
    loss.backward()
    opt_h.step()
    return loss


def eager_step():
    opt_e.zero_grad()
    loss = eager_loss(ref, x, y)
    loss.backward()
    opt_e.step()
    return loss


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


# warm-up of both paths; the first steps' losses must agree
lh = [float(hip_step()) for _ in range(3)]
le = [float(eager_step()) for _ in range(3)]
err = max(abs(a - b) / (1 + abs(b)) for a, b in zip(lh, le))
assert err <= 1e-4, (lh, le)
res = {"batch": B, "channels": C, "length": L, "classes": args.classes, "runs": args.runs,
       "device": torch.cuda.get_device_name(0), "peak_tf_fp32_mfma": PEAK_TF,
       "hip_vs_eager_loss_err": err, "ms": {}, "tflops": {}}
res["ms"]["hip_step"], res["ms"]["eager_step"] = alternate(hip_step, eager_step)

# every launch alone, on the activations of one forward
macs = [C * 8 * 128, 128 * 5 * 256, 256 * 3 * 128]
with torch.no_grad():
    h = x
    for i, blk in enumerate(fcn.layers):
        conv, bn = blk.layers[0], blk.layers[1]
        w, b, K, n = conv.weight, conv.bias, conv.weight.shape[2], B * L
        last = i == 2
        u, part = ft.conv_train_fwd(h, w, b)
        st = ft.bn_finish(part, n, bn.weight, bn.bias, bn.eps, 0.0)  # momentum 0: statistics stay
        yv, gap = ft.bn_relu(u, st, y=not last, gap=last)
        up = torch.randn_like(u) if not last else None
        df = torch.randn(B, u.shape[1], device=dev) if last else None
        du = ft.bn_relu_bwd(u, st, dy=up, dfeat=df)
        dw, db, dg, dbe = torch.empty_like(w), torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)
        hp = pad_same(h, K)
        pairs = {
            "conv_fwd": (lambda: ft.conv_train_fwd(h, w, b), lambda: F.conv1d(pad_same(h, K), w, b)),
            "bn_relu_fwd": (lambda: ft.bn_relu(u, ft.bn_finish(part, n, bn.weight, bn.bias, bn.eps, 0.0),
                                               y=not last, gap=last),
                            (lambda: F.relu(F.batch_norm(u, None, None, bn.weight, bn.bias, True, 0.0, bn.eps)).mean(-1))
                            if last else
                            (lambda: F.relu(F.batch_norm(u, None, None, bn.weight, bn.bias, True, 0.0, bn.eps)))),
            "conv_wgrad": (lambda: ft.conv_wgrad(du, h, K, dw, db),
                           lambda: (torch.nn.grad.conv1d_weight(hp, w.shape, du), du.sum(dim=(0, 2)))),
        }
        if i > 0:
            pairs["conv_dgrad"] = (lambda: ft.conv_dgrad(du, w),
                                   lambda: torch.nn.grad.conv1d_input(hp.shape, w, du))
        with torch.enable_grad():
            uu = u.clone().requires_grad_(True)
            gg, bb = bn.weight.detach().clone().requires_grad_(True), bn.bias.detach().clone().requires_grad_(True)
            out = F.relu(F.batch_norm(uu, None, None, gg, bb, True, 0.0, bn.eps))
            out = out.mean(-1) if last else out
        upstream = df if last else up
        pairs["bn_relu_bwd"] = (
            lambda: ft.bn_relu_bwd(u, st, dy=up, dfeat=df, dgamma=dg, dbeta=dbe),
            lambda: torch.autograd.grad(out, (uu, gg, bb), upstream, retain_graph=True))
        for name, (fh, fe) in pairs.items():
            fh(), fe()
            hip, eager = alternate(fh, fe)
            res["ms"][f"hip_{name}{i + 1}"], res["ms"][f"eager_{name}{i + 1}"] = hip, eager
            if name.startswith("conv"):
                res["tflops"][f"hip_{name}{i + 1}"] = 2.0 * macs[i] * L * B / (hip["median"] * 1e-3) / 1e12
        h = yv
    feat = gap
    fw, fb = fcn.final.weight, fcn.final.bias
    dfw, dfb = torch.empty_like(fw), torch.empty_like(fb)
    _, _, dlog, _ = ft.head_ce(feat, fw, fb, y)
    f2, w2, b2 = (t.detach().clone().requires_grad_(True) for t in (feat, fw, fb))

    def eager_head():
        with torch.enable_grad():
            return torch.autograd.grad(F.cross_entropy(F.linear(f2, w2, b2), y), (f2, w2, b2))

    res["ms"]["hip_head"], res["ms"]["eager_head"] = alternate(
        lambda: (ft.head_ce(feat, fw, fb, y), ft.head_wgrad(dlog, feat, dfw, dfb)), eager_head)

flops = 2.0 * L * B * (2 * sum(macs) + macs[1] + macs[2])
res["flops_per_step"] = flops
for k in ("hip_step", "eager_step"):
    res["tflops"][k] = flops / (res["ms"][k]["median"] * 1e-3) / 1e12
res["share_of_peak"] = {k: v / PEAK_TF for k, v in res["tflops"].items()}
res["eager_over_hip_step"] = res["ms"]["eager_step"]["median"] / res["ms"]["hip_step"]["median"]
res["slower_than_eager"] = sorted(
    k[4:] for k, v in res["ms"].items()
    if k.startswith("hip_") and v["median"] > res["ms"]["eager_" + k[4:]]["median"])
for k, v in res["ms"].items():
    print(f"{k:22s} median {v['median']:9.3f} ms  (min {v['min']:.3f}, max {v['max']:.3f})", flush=True)
for k, v in res["tflops"].items():
    print(f"{k:22s} {v:8.2f} TF = {100 * v / PEAK_TF:5.1f} % of {PEAK_TF:.0f} TF", flush=True)
print("slower than eager:", res["slower_than_eager"], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
