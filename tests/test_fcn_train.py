"""The supervised FCN's training step (timevqvae.hip.fcn_train, FCNBaseline.loss;
csrc/tvq_fcn_train.hip): every op against a float64 torch statement on the CPU, the whole
network against the reference module's float64 step (tests/golden/g18_fcn_train.npz) and
against the same statement at other shapes, and the autograd contract (determinism,
accumulation, frozen parameters, the optimizer's flat gradient sink).

Bounds (fcn_train_ref): per tensor max|got - ref| <= 2e-5 max|ref|; the conv-bias gradient,
whose true value is 0 in front of a training BatchNorm, per channel |got - ref| <= 2e-5
sum_{b,l} |du_ref|.  `test_torch_fp32_is_inside_every_bound` shows on the CPU that fp32
arithmetic can meet them at the shapes used here."""
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, golden
from fcn_train_ref import (REL, close, close_bias_grad, conv_bias_keys, conv_same, err_of,
                           ref_step)
from make_golden_fcn import CASES, fcn_input, fcn_state
from make_golden_fcn_train import DENSE, N_SAMPLE, TARGET_SEED, fcn_targets, sample_index

TRAIN_ENTRIES = {
    "tvq_fcn_stats_size", "tvq_fcn_conv_train_fwd", "tvq_fcn_bn_finish", "tvq_fcn_bn_relu",
    "tvq_fcn_head_ce_workspace", "tvq_fcn_head_ce", "tvq_fcn_head_wgrad",
    "tvq_fcn_bn_bwd_workspace", "tvq_fcn_bn_relu_bwd", "tvq_fcn_pack_weight_t",
    "tvq_fcn_conv_dgrad", "tvq_fcn_conv_wgrad_workspace", "tvq_fcn_conv_wgrad",
}
# shapes the golden lacks: (classes, weight seed, input seed, x shape)
EXTRA = {"tiny": (2, 181, 1181, (2, 1, 5)), "odd": (3, 182, 1182, (3, 4, 129)),
         "wide": (5, 183, 1183, (5, 6, 200))}
# the shapes of the issue's fp32-on-the-CPU measurement
FP32_SHAPES = [(3, 191, (6, 3, 40)), (5, 192, (5, 6, 130)), (2, 193, (2, 1, 5))]


# ------------------------------------------------------------------------------------ CPU
def test_header_declares_the_training_entry_points():
    text = open(os.path.join(ROOT, "include", "tvq_fcn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(tvq_[A-Za-z0-9_]+)\s*\(", text))
    assert TRAIN_ENTRIES <= names, TRAIN_ENTRIES - names
    from timevqvae.hip._native import EXTRA_SIGNATURES
    assert TRAIN_ENTRIES <= set(EXTRA_SIGNATURES)


def test_golden_has_the_generators_cases_and_keys():
    g = golden("g18_fcn_train.npz")
    assert list(g["names"]) == list(CASES)
    for name, (cin, classes, wseed, xseed, shape) in CASES.items():
        assert [int(v) for v in g[f"{name}_meta"]] == [cin, classes, wseed, xseed, TARGET_SEED + xseed]
        y = g[f"{name}_y"]
        assert np.array_equal(y, fcn_targets(xseed, classes, shape[0]))
        assert y[0] == 0 and y[-1] == classes - 1 and y.dtype == np.int64
        assert g[f"{name}_logits"].shape == (shape[0], classes)
        assert list(g[f"{name}_nbt"]) == [101, 101, 101]
        sd = fcn_state(cin, classes, wseed)
        for k in DENSE:
            assert g[f"{name}_g_{k}"].shape == tuple(sd[k].shape), k
        for i in (1, 2):
            numel = sd[f"layers.{i}.layers.0.weight"].numel()
            assert np.array_equal(g[f"{name}_idx{i}"], sample_index(i, numel))
            assert g[f"{name}_val{i}"].shape == (N_SAMPLE,) and g[f"{name}_stat{i}"].shape == (3,)
        for i in range(3):
            assert g[f"{name}_absdu{i}"].shape == g[f"{name}_rm{i}"].shape == g[f"{name}_rv{i}"].shape


def test_golden_is_what_the_float64_statement_gives():
    """the tests' own float64 statement reproduces the reference module's stored step (case c)"""
    g = golden("g18_fcn_train.npz")
    cin, classes, wseed, xseed, shape = CASES["c"]
    r = ref_step(fcn_state(cin, classes, wseed), cin, classes, fcn_input(xseed, shape), g["c_y"])
    assert abs(float(r["loss"]) - float(g["c_loss"])) <= 1e-12
    for k in DENSE:
        if k not in conv_bias_keys():
            assert err_of(r["grads"][k], g[f"c_g_{k}"])[0] <= 1e-12 * (1 + err_of(r["grads"][k], g[f"c_g_{k}"])[1])


def test_cpu_input_and_eval_mode_are_refused():
    from timevqvae.hip import NativeError
    from timevqvae.models import FCNBaseline
    fcn = FCNBaseline(3, 4).train()
    with pytest.raises(NativeError):
        fcn.loss(torch.zeros(2, 3, 16), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="training mode"):
        fcn.eval().loss(torch.zeros(2, 3, 16), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="FCNBaseline training is not on the HIP path"):
        fcn.train()(torch.zeros(2, 3, 16))


def test_train_drops_the_eval_fold_cache():
    from timevqvae.models import FCNBaseline
    fcn = FCNBaseline(3, 4)
    fcn.__dict__["_fcn_fold"] = {0: "stale"}
    fcn.eval()
    assert "_fcn_fold" not in fcn.__dict__


@pytest.mark.parametrize("classes,seed,shape", FP32_SHAPES)
def test_torch_fp32_is_inside_every_bound(classes, seed, shape):
    """torch fp32 on the CPU against torch fp64: an fp32 implementation can meet every bound
    the GPU tests assert, at these shapes."""
    sd = fcn_state(shape[1], classes, seed)
    x, y = fcn_input(seed + 1000, shape), fcn_targets(seed, classes, shape[0])
    r64 = ref_step(sd, shape[1], classes, x, y)
    r32 = ref_step(sd, shape[1], classes, x, y, torch.float32)
    close(r32["loss"], r64["loss"], "loss")
    close(r32["logits"], r64["logits"], "logits")
    for k, g in r64["grads"].items():
        if k in conv_bias_keys():
            close_bias_grad(r32["grads"][k], g, r64["absdu"][int(k.split(".")[1])], k)
        else:
            close(r32["grads"][k], g, k)
    for k, v in r64["state"].items():
        if "running" in k:
            close(r32["state"][k], v, k)


# ------------------------------------------------------------------------------------ GPU ops
@functools.lru_cache(maxsize=None)
def _conv_case(K, Ci, Co, L, B):
    g = torch.Generator().manual_seed(2000 * K + 100 * Ci + Co + L + B)
    x = torch.cumsum(0.1 * torch.randn(B, Ci, L, generator=g), -1)
    w = (torch.rand(Co, Ci, K, generator=g) * 2 - 1) / (Ci * K) ** 0.5
    b = torch.rand(Co, generator=g) - 0.5
    gamma, beta = torch.rand(Co, generator=g) + 0.5, torch.rand(Co, generator=g) - 0.5
    rm, rv = torch.rand(Co, generator=g) - 0.5, torch.rand(Co, generator=g) + 0.5
    u = conv_same(x.double(), w.double(), b.double())
    return x, w, b, gamma, beta, rm, rv, u


# (K, Ci, Co, L, B): L < K; L = 127 / 128 / 129 (one tile, its edge, two tiles); Ci K odd (15,
# 3); Co = 32; the three layers' (K, Ci, Co); B L = 2 both ways
CONV_CASES = [
    (8, 3, 32, 5, 2), (8, 6, 128, 127, 2), (5, 128, 256, 128, 1), (3, 256, 128, 129, 2),
    (5, 3, 32, 65, 2), (3, 1, 32, 7, 3), (8, 1, 32, 1, 2), (3, 1, 32, 2, 1), (2, 5, 64, 200, 2),
]


@pytest.mark.gpu
@pytest.mark.parametrize("K,Ci,Co,L,B", CONV_CASES)
def test_conv_train_fwd_and_statistics_vs_float64(K, Ci, Co, L, B, cuda):
    from timevqvae.hip import fcn_train as ft
    x, w, b, gamma, beta, rm, rv, ur = _conv_case(K, Ci, Co, L, B)
    u, part = ft.conv_train_fwd(x.to(cuda), w.to(cuda), b.to(cuda))
    assert u.shape == (B, Co, L) and part.shape == (2, Co, B * ((L + 127) // 128))
    close(u, ur, "u")
    # a sample's row depends on neither the batch nor the grid
    u1, _ = ft.conv_train_fwd(x[B - 1:].to(cuda), w.to(cuda), b.to(cuda))
    assert torch.equal(u1, u[B - 1:])
    n, eps, mom = B * L, 1e-5, 0.1
    rm_d, rv_d = rm.to(cuda), rv.to(cuda)
    nbt = torch.tensor(7, dtype=torch.int64, device=cuda)
    stats = ft.bn_finish(part, n, gamma.to(cuda), beta.to(cuda), eps, mom, rm_d, rv_d, nbt)
    # the statistics' input is the float32 u the kernel stored (with B L = 2 the variance of
    # the float64 u is a difference that u's own rounding already moves by more than REL)
    u64 = u.double().cpu()
    mean, var = u64.mean(dim=(0, 2)), u64.var(dim=(0, 2), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    close(stats[0], mean, "mean")
    close(stats[1], rstd, "rstd")
    close(stats[2], gamma.double() * rstd, "scale")
    close(stats[3], beta.double() - mean * gamma.double() * rstd, "shift")
    close(rm_d, 0.9 * rm.double() + 0.1 * mean, "running_mean")
    close(rv_d, 0.9 * rv.double() + 0.1 * var * n / (n - 1), "running_var")
    assert int(nbt) == 8


@pytest.mark.gpu
def test_one_value_per_channel_is_refused(cuda):
    from timevqvae.models import FCNBaseline
    fcn = FCNBaseline(1, 2).to(cuda).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        fcn.loss(torch.zeros(1, 1, 1, device=cuda), torch.zeros(1, dtype=torch.int64, device=cuda))


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,L", [(3, 32, 5), (2, 128, 127), (1, 64, 128), (2, 32, 129), (2, 40, 300)])
def test_bn_relu_apply_and_gap(B, C, L, cuda):
    from timevqvae.hip import fcn_train as ft
    g = torch.Generator().manual_seed(B + C + L)
    u = torch.randn(B, C, L, generator=g)
    stats = torch.stack([torch.zeros(C), torch.ones(C), torch.rand(C, generator=g) + 0.5,
                         torch.rand(C, generator=g) - 0.5])
    yr = torch.relu(u.double() * stats[2].double()[None, :, None] + stats[3].double()[None, :, None])
    y, gap = ft.bn_relu(u.to(cuda), stats.to(cuda), y=True, gap=True)
    close(y, yr, "y")
    close(gap, yr.mean(-1), "gap")
    none, alone = ft.bn_relu(u.to(cuda), stats.to(cuda), y=False, gap=True)
    assert none is None and torch.equal(alone, gap)
    only, none = ft.bn_relu(u.to(cuda), stats.to(cuda), y=True, gap=False)
    assert none is None and torch.equal(only, y)


@pytest.mark.gpu
def test_bn_relu_gap_has_the_eval_kernels_order(cuda):
    """the pooled features of the training apply are the eval kernel's, bit for bit, when both
    see the same pre-activation: a 1-tap identity conv with scale 1, shift 0 passes u through"""
    from timevqvae.hip import fcn_train as ft
    from timevqvae.hip.fcn import conv_bn_relu
    g = torch.Generator().manual_seed(9)
    u = torch.randn(2, 32, 300, generator=g).to(cuda)
    w = torch.eye(32).reshape(32, 32, 1).to(cuda)
    one, zero = torch.ones(32, device=cuda), torch.zeros(32, device=cuda)
    _, gap_eval = conv_bn_relu(u, w, one, zero, y=False, gap=True)
    stats = torch.stack([zero, one, one, zero])
    _, gap_train = ft.bn_relu(u, stats, y=False, gap=True)
    assert torch.equal(gap_eval, gap_train)


@pytest.mark.gpu
@pytest.mark.parametrize("classes", [1, 2, 37])
def test_head_cross_entropy_vs_float64(classes, cuda):
    from timevqvae.hip import fcn_train as ft
    B, D = 5, 128
    g = torch.Generator().manual_seed(classes)
    feat, w = torch.rand(B, D, generator=g), torch.rand(classes, D, generator=g) * 2 - 1
    b = torch.rand(classes, generator=g) - 0.5
    y = torch.randint(0, classes, (B,), generator=g)
    y[0], y[-1] = 0, classes - 1
    f64, w64, b64 = (t.double().requires_grad_(True) for t in (feat, w, b))
    lr = F.linear(f64, w64, b64)
    lr.retain_grad()
    loss_r = F.cross_entropy(lr, y)
    loss_r.backward()
    logits, loss, dlogits, dfeat = ft.head_ce(feat.to(cuda), w.to(cuda), b.to(cuda), y.to(cuda))
    dw, db = torch.empty(classes, D, device=cuda), torch.empty(classes, device=cuda)
    ft.head_wgrad(dlogits, feat.to(cuda), dw, db)
    close(logits, lr.detach(), "logits")
    if classes == 1:
        assert float(loss) == 0.0
        assert not dlogits.any() and not dfeat.any() and not dw.any() and not db.any()
        return
    close(loss, loss_r.detach(), "loss")
    close(dlogits, lr.grad, "dlogits")
    close(dfeat, f64.grad, "dfeat")
    close(dw, w64.grad, "dW")
    close(db, b64.grad, "db")
    twice_w, twice_b = dw.clone(), db.clone()
    ft.head_wgrad(dlogits, feat.to(cuda), twice_w, twice_b, accumulate=True)
    assert torch.equal(twice_w, 2 * dw) and torch.equal(twice_b, 2 * db)


@pytest.mark.gpu
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("B,C,L", [(3, 32, 5), (2, 33, 130)])
def test_bn_relu_backward_vs_float64(B, C, L, broadcast, cuda):
    """channel 0 has gamma = beta = 0 (v == 0 everywhere: no gradient passes, as in torch),
    channel 1 has beta << 0 (every position dead)"""
    from timevqvae.hip import fcn_train as ft
    g = torch.Generator().manual_seed(B * C + L + broadcast)
    u = torch.randn(B, C, L, generator=g) + 0.3
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    gamma[0] = beta[0] = 0.0
    beta[1] = -100.0
    up = torch.randn(B, C, generator=g) if broadcast else torch.randn(B, C, L, generator=g)
    eps = 1e-5
    u64, g64, b64 = (t.double().requires_grad_(True) for t in (u, gamma, beta))
    yr = torch.relu(F.batch_norm(u64, None, None, g64, b64, True, 0.1, eps))
    (yr.mean(-1) if broadcast else yr).backward(up.double())
    mean, var = u.double().mean(dim=(0, 2)), u.double().var(dim=(0, 2), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * rstd
    stats = torch.stack([mean, rstd, scale, beta.double() - mean * scale]).float().to(cuda)
    dg, db = torch.empty(C, device=cuda), torch.empty(C, device=cuda)
    kw = {"dfeat": up.to(cuda)} if broadcast else {"dy": up.to(cuda)}
    du = ft.bn_relu_bwd(u.to(cuda), stats, dgamma=dg, dbeta=db, **kw)
    close(du, u64.grad, "du")
    close(dg, g64.grad, "dgamma")
    close(db, b64.grad, "dbeta")
    assert not du[:, :2].any() and not dg[:2].any() and not db[:2].any()
    assert not u64.grad[:, :2].any()
    # the gradients may be skipped, and accumulate adds
    du2 = ft.bn_relu_bwd(u.to(cuda), stats, **kw)
    assert torch.equal(du2, du)
    dg2, db2 = dg.clone(), db.clone()
    ft.bn_relu_bwd(u.to(cuda), stats, dgamma=dg2, dbeta=db2, accumulate=True, **kw)
    assert torch.equal(dg2, 2 * dg) and torch.equal(db2, 2 * db)


# (K, Ci, Co, L, B): K = 8 and K = 2 have different paddings on the two sides, so they fail with
# the forward's left padding; L < K; more than one position tile
DGRAD_CASES = [(8, 32, 32, 40, 2), (5, 32, 64, 130, 1), (3, 64, 32, 7, 2), (2, 32, 32, 5, 2),
               (1, 32, 32, 9, 1), (8, 32, 32, 3, 2), (2, 128, 32, 129, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("K,Ci,Co,L,B", DGRAD_CASES)
def test_conv_data_gradient_vs_float64(K, Ci, Co, L, B, cuda):
    from timevqvae.hip import fcn_train as ft
    g = torch.Generator().manual_seed(3000 * K + Ci + Co + L + B)
    w = (torch.rand(Co, Ci, K, generator=g) * 2 - 1) / (Ci * K) ** 0.5
    du = torch.randn(B, Co, L, generator=g)
    h = torch.zeros(B, Ci, L, dtype=torch.float64, requires_grad=True)
    conv_same(h, w.double()).backward(du.double())
    dh = ft.conv_dgrad(du.to(cuda), w.to(cuda))
    assert dh.shape == (B, Ci, L)
    close(dh, h.grad, "dh")


# (K, Ci, Co, L, B): layer 1's Ci = 1, 3, 6 (padded to the MFMA step); the other two layers'
# (K, Ci, Co) with L off the 64-position stage; 300 samples over the plan's 256 splits (uneven
# ranges); L < K
WGRAD_CASES = [(8, 1, 128, 40, 3), (8, 3, 128, 40, 3), (8, 6, 128, 70, 2), (5, 128, 256, 65, 2),
               (3, 256, 128, 40, 2), (8, 3, 32, 3, 300), (2, 5, 32, 129, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("K,Ci,Co,L,B", WGRAD_CASES)
def test_conv_weight_and_bias_gradient_vs_float64(K, Ci, Co, L, B, cuda):
    from timevqvae.hip import fcn_train as ft
    from timevqvae.hip._native import plan_trace
    g = torch.Generator().manual_seed(4000 * K + Ci + Co + L + B)
    h = torch.cumsum(0.1 * torch.randn(B, Ci, L, generator=g), -1)
    du = torch.randn(B, Co, L, generator=g)
    w = torch.zeros(Co, Ci, K, dtype=torch.float64, requires_grad=True)
    conv_same(h.double(), w).backward(du.double())
    dw, db = torch.empty(Co, Ci, K, device=cuda), torch.empty(Co, device=cuda)
    with plan_trace() as pt:
        ft.conv_wgrad(du.to(cuda), h.to(cuda), K, dw, db)
    line = pt.has("fcn_wgrad")[0]
    print(line)
    splits = int(re.search(r"splits=(\d+)", line).group(1))
    assert splits == min(B, 256) or splits * -(-Ci * K // 128) * -(-Co // 64) >= 512
    if B >= 2:
        assert splits >= 2
    close(dw, w.grad, "dw")
    close_bias_grad(db, du.double().sum(dim=(0, 2)), du.double().abs().sum(dim=(0, 2)), "db")
    # either output may be skipped; accumulate adds
    only_w = torch.empty_like(dw)
    ft.conv_wgrad(du.to(cuda), h.to(cuda), K, only_w, None)
    only_b = torch.empty_like(db)
    ft.conv_wgrad(du.to(cuda), h.to(cuda), K, None, only_b)
    assert torch.equal(only_w, dw) and torch.equal(only_b, db)
    ft.conv_wgrad(du.to(cuda), h.to(cuda), K, only_w, only_b, accumulate=True)
    assert torch.equal(only_w, 2 * dw) and torch.equal(only_b, 2 * db)


# ------------------------------------------------------------------------------------ whole net
def _module(cin, classes, wseed, cuda, frozen=()):
    from timevqvae.models import FCNBaseline
    fcn = FCNBaseline(cin, classes)
    fcn.load_state_dict(fcn_state(cin, classes, wseed), strict=True)
    fcn = fcn.to(cuda).train()
    for k, p in fcn.named_parameters():
        p.requires_grad_(k not in frozen)
    return fcn


def _step(cin, classes, wseed, x, y, cuda, frozen=(), flat=False, times=1):
    """loss, logits, the gradients and the state after `times` loss / backward rounds"""
    fcn = _module(cin, classes, wseed, cuda, frozen)
    if flat:
        from timevqvae.hip.optim import FusedAdamW
        opt = FusedAdamW(fcn.parameters(), lr=1e-3)
        opt.zero_grad()
    xd, yd = torch.as_tensor(x).to(cuda), torch.as_tensor(y).to(cuda)
    for _ in range(times):
        loss, logits = fcn.loss(xd, yd)
        loss.backward()
    grads = {k: (p.grad.detach().cpu().clone() if p.grad is not None else None)
             for k, p in fcn.named_parameters()}
    return {"loss": loss.detach().cpu(), "logits": logits.cpu(), "grads": grads,
            "state": {k: v.detach().cpu().clone() for k, v in fcn.state_dict().items()}}


@functools.lru_cache(maxsize=None)
def _extra(name):
    classes, wseed, xseed, shape = EXTRA[name]
    return fcn_input(xseed, shape), fcn_targets(xseed, classes, shape[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_training_step_matches_the_reference_golden(name, cuda):
    g = golden("g18_fcn_train.npz")
    cin, classes, wseed, xseed, shape = CASES[name]
    r = _step(cin, classes, wseed, fcn_input(xseed, shape), g[f"{name}_y"], cuda)
    assert r["loss"].dim() == 0
    close(r["loss"], g[f"{name}_loss"], "loss")
    close(r["logits"], g[f"{name}_logits"], "logits")
    for i in range(3):
        close(r["state"][f"layers.{i}.layers.1.running_mean"], g[f"{name}_rm{i}"], f"running_mean {i}")
        close(r["state"][f"layers.{i}.layers.1.running_var"], g[f"{name}_rv{i}"], f"running_var {i}")
        assert int(r["state"][f"layers.{i}.layers.1.num_batches_tracked"]) == 101
    for k in DENSE:
        if k in conv_bias_keys():
            i = int(k.split(".")[1])
            close_bias_grad(r["grads"][k], g[f"{name}_g_{k}"], g[f"{name}_absdu{i}"], k)
        else:
            close(r["grads"][k], g[f"{name}_g_{k}"], k)
    for i in (1, 2):
        got = r["grads"][f"layers.{i}.layers.0.weight"].double().reshape(-1)
        s1, s2, top = (float(v) for v in g[f"{name}_stat{i}"])
        d = float((got[g[f"{name}_idx{i}"]] - torch.from_numpy(g[f"{name}_val{i}"])).abs().max())
        print(f"conv weight {i}: sampled max err {d:.3e} = {d / top:.2e} of max|ref| {top:.3e}")
        assert d <= REL * top
        # every entry within e = REL max|ref| moves the sum by <= numel e, the sum of squares
        # by <= 2 e sum|g| + numel e^2
        e, n = REL * top, got.numel()
        assert abs(float(got.sum()) - s1) <= n * e
        assert abs(float((got * got).sum()) - s2) <= 2 * e * float(got.abs().sum()) + n * e * e
        assert float(got.abs().max()) <= top * (1 + REL) and float(got.abs().max()) >= top * (1 - REL)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EXTRA))
def test_training_step_vs_float64_at_other_shapes(name, cuda):
    classes, wseed, xseed, shape = EXTRA[name]
    x, y = _extra(name)
    sd = fcn_state(shape[1], classes, wseed)
    ref = ref_step(sd, shape[1], classes, x, y)
    r = _step(shape[1], classes, wseed, x, y, cuda)
    close(r["loss"], ref["loss"], "loss")
    close(r["logits"], ref["logits"], "logits")
    for k, gr in ref["grads"].items():
        if k in conv_bias_keys():
            close_bias_grad(r["grads"][k], gr, ref["absdu"][int(k.split(".")[1])], k)
        else:
            close(r["grads"][k], gr, k)
    for k, v in ref["state"].items():
        if "running" in k:
            close(r["state"][k], v, k)
        if "num_batches" in k:
            assert int(r["state"][k]) == int(v) == 101


def _same(a, b):
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["logits"], b["logits"])
    for k, g in a["grads"].items():
        assert (g is None) == (b["grads"][k] is None), k
        assert g is None or torch.equal(g, b["grads"][k]), k
    for k, v in a["state"].items():
        assert torch.equal(v, b["state"][k]), k


@pytest.mark.gpu
def test_two_runs_are_bitwise_equal_and_backward_accumulates(cuda):
    classes, wseed, _, shape = EXTRA["wide"]
    x, y = _extra("wide")
    a = _step(shape[1], classes, wseed, x, y, cuda)
    _same(a, _step(shape[1], classes, wseed, x, y, cuda))
    # a second loss / backward without zero_grad doubles every gradient exactly (the batch
    # statistics, hence the gradients, do not depend on the running statistics)
    two = _step(shape[1], classes, wseed, x, y, cuda, times=2)
    for k, g in a["grads"].items():
        assert torch.equal(two["grads"][k], 2 * g), k
    assert int(two["state"]["layers.0.layers.1.num_batches_tracked"]) == 102


@pytest.mark.gpu
def test_flat_gradient_sink_equals_autograds_return(cuda):
    classes, wseed, _, shape = EXTRA["odd"]
    x, y = _extra("odd")
    plain = _step(shape[1], classes, wseed, x, y, cuda)
    _same(plain, _step(shape[1], classes, wseed, x, y, cuda, flat=True))
    two = _step(shape[1], classes, wseed, x, y, cuda, flat=True, times=2)
    for k, g in plain["grads"].items():
        assert torch.equal(two["grads"][k], 2 * g), k


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [False, True])
def test_frozen_parameters_get_no_gradient(flat, cuda):
    from timevqvae.hip._native import plan_trace
    classes, wseed, _, shape = EXTRA["odd"]
    x, y = _extra("odd")
    plain = _step(shape[1], classes, wseed, x, y, cuda)
    frozen = tuple(conv_bias_keys())
    r = _step(shape[1], classes, wseed, x, y, cuda, frozen=frozen, flat=flat)
    for k, g in plain["grads"].items():
        if k in frozen:
            assert r["grads"][k] is None
        else:
            assert torch.equal(r["grads"][k], g), k
    # frozen conv weights and biases: no weight-gradient launch at all
    convs = frozen + tuple(f"layers.{i}.layers.0.weight" for i in range(3))
    with plan_trace() as pt:
        r = _step(shape[1], classes, wseed, x, y, cuda, frozen=convs, flat=flat)
    assert not pt.has("fcn_wgrad") and len(pt.has("fcn_conv_dgrad")) == 2
    for k, g in plain["grads"].items():
        assert (r["grads"][k] is None) if k in convs else torch.equal(r["grads"][k], g), k
