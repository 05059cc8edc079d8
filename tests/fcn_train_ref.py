"""Float64 / float32 torch statements of the supervised FCN's training step on the CPU, shared by
tests/test_fcn_train.py and tests/test_fcn_trainer.py (no test in here).

RefFCN has the reference's state-dict keys (load `fcn_state` into it) and is plain torch:
F.pad + F.conv1d (TensorFlow "same": (K-1)//2 on the left), nn.BatchNorm1d, ReLU, the mean
over positions, nn.Linear; the loss is torch.nn.CrossEntropyLoss."""
import torch
import torch.nn.functional as F
from torch import nn

REL = 2e-5        # per tensor: max|got - ref| <= REL max|ref| (tests/test_fcn.py)
STEP_REL = 1e-4   # multi-step loss: |d| <= STEP_REL (1 + |ref|) (tests/test_stage3.py)


def conv_same(h, w, b=None):
    K = w.shape[2]
    pl = (K - 1) // 2
    return F.conv1d(F.pad(h, (pl, K - 1 - pl)), w, b)


class RefBlock(nn.Module):
    def __init__(self, ci, co, k):
        super().__init__()
        self.layers = nn.Sequential(nn.Conv1d(ci, co, k), nn.BatchNorm1d(co), nn.ReLU())

    def forward(self, x):
        conv, bn, act = self.layers
        self.u = conv_same(x, conv.weight, conv.bias)
        if self.u.requires_grad:
            self.u.retain_grad()
        return act(bn(self.u))


class RefFCN(nn.Module):
    def __init__(self, cin, classes):
        super().__init__()
        self.layers = nn.Sequential(RefBlock(cin, 128, 8), RefBlock(128, 256, 5), RefBlock(256, 128, 3))
        self.final = nn.Linear(128, classes)

    def forward(self, x, return_feature_vector=False):
        f = self.layers(x).mean(-1)
        return f if return_feature_vector else self.final(f)


def ref_fcn(sd, cin, classes, dtype=torch.float64):
    m = RefFCN(cin, classes)
    m.load_state_dict(sd, strict=True)
    return m.to(dtype).train()


def ref_step(sd, cin, classes, x, y, dtype=torch.float64):
    """One training forward / backward: dict with loss, logits, grads (by state-dict key),
    absdu (per layer, sum_{b,l} |du| per channel) and the state dict after the step."""
    m = ref_fcn(sd, cin, classes, dtype)
    logits = m(torch.as_tensor(x).to(dtype))
    loss = F.cross_entropy(logits, torch.as_tensor(y).reshape(-1))
    loss.backward()
    return {"loss": loss.detach().double(), "logits": logits.detach().double(),
            "grads": {k: p.grad.double() for k, p in m.named_parameters()},
            "absdu": [blk.u.grad.double().abs().sum(dim=(0, 2)) for blk in m.layers],
            "state": {k: v.detach().clone() for k, v in m.state_dict().items()}}


def conv_bias_keys():
    return [f"layers.{i}.layers.0.bias" for i in range(3)]


def err_of(got, ref):
    """(max|got - ref|, max|ref|) in float64 on the CPU"""
    ref = torch.as_tensor(ref).double()
    got = torch.as_tensor(got).detach().double().cpu().reshape(ref.shape)
    return float((got - ref).abs().max()), float(ref.abs().max())


def close(got, ref, what, rel=REL):
    err, top = err_of(got, ref)
    print(f"{what}: max err {err:.3e} = {err / max(top, 1e-300):.2e} of max|ref| {top:.3e}")
    assert err <= rel * top, f"{what}: {err:.3e} > {rel} * {top:.3e}"


def close_bias_grad(got, ref, absdu, what):
    """the conv-bias gradient in front of a training BatchNorm is 0 up to rounding: per channel
    |got - ref| <= REL sum_{b,l} |du_ref|"""
    ref = torch.as_tensor(ref).double()
    d = (torch.as_tensor(got).detach().double().cpu().reshape(ref.shape) - ref).abs()
    bound = REL * torch.as_tensor(absdu).double()
    worst = float((d / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |d| {float(d.max()):.3e}, worst share of the bound {worst:.2e}")
    assert bool((d <= bound).all()), f"{what}: {float(d.max()):.3e} outside REL * sum|du|"
