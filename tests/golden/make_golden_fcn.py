"""Generate the G17 golden (supervised FCN extractor: features, logits, softmax, IS) from the
REFERENCE timevqvae/models/fcn.py FCNBaseline and evaluation/eval_utils.py
calculate_inception_score.

Runs only where the reference checkout exists (the build container); fcn.py imports only torch
and is loaded by path.  Only the .npz output is committed:

    tests/golden/g17_fcn.npz
      names                      the case names
      <case>_meta                in_channels, classes, weight seed, input seed
      <case>_x                   the input (b, c, l) float32: random walks cumsum(0.1 N(0,1))
      <case>_feat32, _logits32   the reference module in float32 on the CPU
      <case>_feat64, _logits64   the same module .double() on the float64 input
      <case>_probs               softmax of _logits64
      <case>_sum, <case>_sq      float64 sum and sum of squares of every state-dict tensor, in
                                 the order of <case>_keys
      a_is                       calculate_inception_score(a_probs, n_split=1, shuffle=False)[0]

A full-size FCN has about 268k parameters, more than a committed fixture may hold, so the
weights are not stored: `fcn_state(in_channels, classes, seed)` below rebuilds them from
np.random.default_rng(seed), and the tests import it; the stored sums catch a generator that
drifts.  The BatchNorm statistics are non-trivial (gamma in [0.5, 1.5], beta and running_mean
in +-0.5, running_var in [0.5, 2]) so that the fold is tested.

Cases: a (6 channels, 5 classes, x (7, 6, 200)); b (1, 2, (3, 1, 5)): shorter than the widest
kernel; c (3, 37, (4, 3, 65)).  Asserted here: every row's top-2 logit gap (float64) is >= 1e-3,
so the tests may ask for the reference's argmax on every row.

    python tests/golden/make_golden_fcn.py
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))

CASES = {  # name: (in_channels, classes, weight seed, input seed, x shape)
    "a": (6, 5, 171, 1171, (7, 6, 200)),
    "b": (1, 2, 172, 1172, (3, 1, 5)),
    "c": (3, 37, 173, 1173, (4, 3, 65)),
}
_BLOCKS = ((128, 8), (256, 5), (128, 3))  # (out channels, kernel) of the three ConvBlocks


def fcn_state(in_channels, classes, seed):
    """The state dict of FCNBaseline(in_channels, classes) (reference keys, float32) drawn from
    np.random.default_rng(seed): conv / linear weights and biases uniform in +-1/sqrt(fan_in)
    (the final weight in +-1, for logits that differ), BatchNorm gamma in [0.5, 1.5], beta and
    running_mean in +-0.5, running_var in [0.5, 2], num_batches_tracked = 100."""
    rng = np.random.default_rng(seed)
    sd = {}

    def uni(lo, hi, shape):
        return torch.from_numpy(rng.uniform(lo, hi, shape).astype(np.float32))

    ci = in_channels
    for i, (co, k) in enumerate(_BLOCKS):
        b = 1.0 / np.sqrt(ci * k)
        sd[f"layers.{i}.layers.0.weight"] = uni(-b, b, (co, ci, k))
        sd[f"layers.{i}.layers.0.bias"] = uni(-b, b, (co,))
        sd[f"layers.{i}.layers.1.weight"] = uni(0.5, 1.5, (co,))
        sd[f"layers.{i}.layers.1.bias"] = uni(-0.5, 0.5, (co,))
        sd[f"layers.{i}.layers.1.running_mean"] = uni(-0.5, 0.5, (co,))
        sd[f"layers.{i}.layers.1.running_var"] = uni(0.5, 2.0, (co,))
        sd[f"layers.{i}.layers.1.num_batches_tracked"] = torch.tensor(100, dtype=torch.int64)
        ci = co
    sd["final.weight"] = uni(-1.0, 1.0, (classes, 128))
    sd["final.bias"] = uni(-1.0 / np.sqrt(128), 1.0 / np.sqrt(128), (classes,))
    return sd


def state_sums(sd):
    """(keys, float64 sums, float64 sums of squares) of a state dict, in key order."""
    keys = sorted(sd)
    v = [sd[k].double().numpy() for k in keys]
    return keys, np.array([a.sum() for a in v]), np.array([(a * a).sum() for a in v])


def fcn_input(seed, shape):
    rng = np.random.default_rng(seed)
    return np.cumsum(0.1 * rng.standard_normal(shape), axis=-1).astype(np.float32)


def main():
    sys.path.insert(0, OUT)
    from make_golden import REF, _load
    from make_golden_fid_device import load_eval_utils
    ref = _load("ref_fcn", f"{REF}/models/fcn.py")
    eu = load_eval_utils()
    d = {"names": np.array(list(CASES))}
    for name, (cin, classes, wseed, xseed, shape) in CASES.items():
        sd = fcn_state(cin, classes, wseed)
        x = fcn_input(xseed, shape)
        m = ref.FCNBaseline(cin, classes)
        m.load_state_dict(sd, strict=True)
        m.eval()
        with torch.no_grad():
            xt = torch.from_numpy(x)
            f32, l32 = m(xt, return_feature_vector=True), m(xt)
            m64 = m.double()
            f64, l64 = m64(xt.double(), return_feature_vector=True), m64(xt.double())
        top = torch.sort(l64, dim=-1, descending=True).values
        gap = float((top[:, 0] - top[:, 1]).min()) if classes > 1 else float("inf")
        assert gap >= 1e-3, (name, gap)
        probs = torch.softmax(l64, dim=-1).numpy()
        keys, s1, s2 = state_sums(sd)
        d[f"{name}_meta"] = np.array([cin, classes, wseed, xseed])
        d[f"{name}_x"] = x
        d[f"{name}_feat32"], d[f"{name}_logits32"] = f32.numpy(), l32.numpy()
        d[f"{name}_feat64"], d[f"{name}_logits64"] = f64.numpy(), l64.numpy()
        d[f"{name}_probs"] = probs
        d[f"{name}_keys"], d[f"{name}_sum"], d[f"{name}_sq"] = np.array(keys), s1, s2
        e32 = float((f32.double() - f64).abs().max() / f64.abs().max())
        print(f"{name}: x {shape} top-2 gap {gap:.3e} feat max {float(f64.abs().max()):.3f} "
              f"logit max {float(l64.abs().max()):.3f} cpu fp32 feat err/max {e32:.2e}")
        if name == "a":
            d["a_is"] = np.float64(eu.calculate_inception_score(probs.copy(), n_split=1,
                                                                shuffle=False)[0])
            print(f"a: IS {float(d['a_is']):.6f}")
    path = os.path.join(OUT, "g17_fcn.npz")
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(f"wrote g17_fcn.npz: {size} bytes")


if __name__ == "__main__":
    main()
