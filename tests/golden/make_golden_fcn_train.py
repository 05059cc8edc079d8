"""Generate the G18 golden (supervised FCN training step: loss, logits, running statistics and
gradients) from the REFERENCE timevqvae/models/fcn.py FCNBaseline in `.double().train()` under
torch.nn.CrossEntropyLoss (scripts/train_fcn.py:116-124).

Runs only where the reference checkout exists; fcn.py imports only torch and is loaded by path.
Only the .npz output is committed:

    tests/golden/g18_fcn_train.npz
      names                    the case names: G17's (make_golden_fcn.CASES), the same weights
                               (`fcn_state` seeds) and inputs (`fcn_input` seeds)
      <case>_meta              in_channels, classes, weight seed, input seed, target seed
      <case>_y                 the targets (b,) int64: seeded, y[0] = 0, y[-1] = classes - 1
      <case>_loss, _logits     float64
      <case>_rm<i>, _rv<i>     layer i's running_mean / running_var after the step; _nbt = 101
      <case>_absdu<i>          sum_{b,l} |du| per channel of layer i's conv output: the scale of
                               the conv-bias gradient's bound (its true value is 0)
      <case>_g_<key>           dense float64 gradient of every BatchNorm gamma / beta, conv bias,
                               final.* and layer 0's conv weight
      <case>_idx<i>, _val<i>,  for the conv weights of layers 1 and 2: 2048 seeded flat indices
      <case>_stat<i>           with the gradient there, and (sum, sum of squares, max|g|)

    python tests/golden/make_golden_fcn_train.py
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)

from make_golden_fcn import CASES, fcn_input, fcn_state  # noqa: E402

TARGET_SEED = 5000   # + the case's input seed
SAMPLE_SEED = 7000   # + the layer index
N_SAMPLE = 2048
DENSE = ([f"layers.{i}.layers.{j}.{n}" for i in range(3) for j, n in ((0, "bias"), (1, "weight"), (1, "bias"))]
         + ["layers.0.layers.0.weight", "final.weight", "final.bias"])


def fcn_targets(xseed, classes, b):
    y = np.random.default_rng(TARGET_SEED + xseed).integers(0, classes, b).astype(np.int64)
    y[0], y[-1] = 0, classes - 1
    return y


def sample_index(layer, numel):
    return np.random.default_rng(SAMPLE_SEED + layer).integers(0, numel, N_SAMPLE).astype(np.int64)


def train_step_f64(module, x, y):
    """One training-mode forward / backward of a reference-shaped FCNBaseline in float64:
    (loss, logits, the conv outputs' gradients)."""
    m = module.double().train()
    us = []

    def keep(_module, _inputs, out):
        out.retain_grad()
        us.append(out)

    hooks = [blk.layers[0].register_forward_hook(keep) for blk in m.layers]
    logits = m(torch.as_tensor(x).double())
    loss = torch.nn.CrossEntropyLoss()(logits, torch.as_tensor(y))
    loss.backward()
    for h in hooks:
        h.remove()
    return loss.detach(), logits.detach(), [u.grad for u in us]


def main():
    from make_golden import REF, _load
    ref = _load("ref_fcn", f"{REF}/models/fcn.py")
    d = {"names": np.array(list(CASES))}
    for name, (cin, classes, wseed, xseed, shape) in CASES.items():
        m = ref.FCNBaseline(cin, classes)
        m.load_state_dict(fcn_state(cin, classes, wseed), strict=True)
        x, y = fcn_input(xseed, shape), fcn_targets(xseed, classes, shape[0])
        loss, logits, dus = train_step_f64(m, x, y)
        d[f"{name}_meta"] = np.array([cin, classes, wseed, xseed, TARGET_SEED + xseed])
        d[f"{name}_y"] = y
        d[f"{name}_loss"], d[f"{name}_logits"] = np.float64(loss), logits.numpy()
        sd = m.state_dict()
        for i in range(3):
            d[f"{name}_rm{i}"] = sd[f"layers.{i}.layers.1.running_mean"].numpy()
            d[f"{name}_rv{i}"] = sd[f"layers.{i}.layers.1.running_var"].numpy()
            d[f"{name}_absdu{i}"] = dus[i].abs().sum(dim=(0, 2)).numpy()
        d[f"{name}_nbt"] = np.array([int(sd[f"layers.{i}.layers.1.num_batches_tracked"]) for i in range(3)])
        grads = {k: p.grad.numpy() for k, p in m.named_parameters()}
        for k in DENSE:
            d[f"{name}_g_{k}"] = grads[k]
        for i in (1, 2):
            g = grads[f"layers.{i}.layers.0.weight"].reshape(-1)
            idx = sample_index(i, g.size)
            d[f"{name}_idx{i}"], d[f"{name}_val{i}"] = idx, g[idx]
            d[f"{name}_stat{i}"] = np.array([g.sum(), (g * g).sum(), np.abs(g).max()])
        print(f"{name}: x {shape} y {y.tolist()} loss {float(loss):.6f} "
              f"max|dw1| {d[f'{name}_stat1'][2]:.3e} max|db_conv0| "
              f"{np.abs(grads['layers.0.layers.0.bias']).max():.2e}")
    path = os.path.join(OUT, "g18_fcn_train.npz")
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(f"wrote g18_fcn_train.npz: {size} bytes")


if __name__ == "__main__":
    main()
