"""The supervised FCN extractor (timevqvae.models.FCNBaseline, timevqvae.hip.fcn,
timevqvae.evaluation.fcn_*; csrc/tvq_fcn.hip): the parameter holder on the CPU, the conv
block and the head op by op against float64 torch statements, the whole network against the
reference module's float64 outputs (tests/golden/g17_fcn.npz), and the places it plugs in.

Bound of every comparison with float64: max|got - ref| <= 2e-5 max|ref| per tensor (the conv
tests' rule, tests/test_resblock.py); it allows any fp32 summation order (torch fp32 on the
CPU sits near 1.2e-7) and nothing else."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from make_golden_fcn import CASES, fcn_state, state_sums

REL = 2e-5

KEYS = {}
for _i, (_ci, _co, _k) in enumerate([(6, 128, 8), (128, 256, 5), (256, 128, 3)]):
    KEYS[f"layers.{_i}.layers.0.weight"] = (_co, _ci, _k)
    KEYS[f"layers.{_i}.layers.0.bias"] = (_co,)
    for _n in ("weight", "bias", "running_mean", "running_var"):
        KEYS[f"layers.{_i}.layers.1.{_n}"] = (_co,)
    KEYS[f"layers.{_i}.layers.1.num_batches_tracked"] = ()
KEYS["final.weight"] = (5, 128)
KEYS["final.bias"] = (5,)


def _fcn(cin, classes, seed, device=None):
    from timevqvae.models import FCNBaseline
    fcn = FCNBaseline(cin, classes)
    fcn.load_state_dict(fcn_state(cin, classes, seed), strict=True)
    fcn.eval()
    return fcn if device is None else fcn.to(device)


# ------------------------------------------------------------------------------------ CPU
def test_state_dict_has_the_reference_keys():
    from timevqvae.models import FCNBaseline
    fcn = FCNBaseline(6, 5)
    sd = fcn.state_dict()
    assert len(KEYS) == 23 and list(sd) == list(KEYS)
    assert {k: tuple(v.shape) for k, v in sd.items()} == KEYS
    assert fcn.input_args == {"in_channels": 6, "num_pred_classes": 5}
    assert FCNBaseline(3).final.weight.shape == (1, 128)


@pytest.mark.parametrize("name", list(CASES))
def test_generated_state_loads_strictly_and_matches_the_golden(name):
    cin, classes, wseed, _, _ = CASES[name]
    g = golden("g17_fcn.npz")
    assert [int(v) for v in g[f"{name}_meta"][:3]] == [cin, classes, wseed]
    sd = fcn_state(cin, classes, wseed)
    keys, s1, s2 = state_sums(sd)
    assert keys == list(g[f"{name}_keys"])
    drift = "fcn_state drifted from the generator that wrote g17_fcn.npz"
    np.testing.assert_allclose(s1, g[f"{name}_sum"], rtol=1e-12, atol=1e-12, err_msg=drift)
    np.testing.assert_allclose(s2, g[f"{name}_sq"], rtol=1e-12, atol=1e-12, err_msg=drift)
    _fcn(cin, classes, wseed)  # strict=True


def test_load_pretrained_fcn_round_trips(tmp_path):
    from timevqvae.evaluation import load_pretrained_FCN
    sd = fcn_state(6, 5, 3)
    torch.save(sd, tmp_path / "fcn.ckpt")
    fcn = load_pretrained_FCN(str(tmp_path / "fcn.ckpt"), 6, 5)
    assert not fcn.training and all(not m.training for m in fcn.modules())
    assert all(not p.requires_grad for p in fcn.parameters())
    got = fcn.state_dict()
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert next(fcn.parameters()).device.type == "cpu"


def test_training_mode_forward_is_refused():
    fcn = _fcn(6, 5, 3).train()
    with pytest.raises(NotImplementedError, match="FCNBaseline training is not on the HIP path"):
        fcn(torch.zeros(2, 6, 16))


def test_cpu_input_is_refused():
    from timevqvae.evaluation import fcn_features
    from timevqvae.hip import NativeError
    fcn = _fcn(6, 5, 3)
    with pytest.raises(NativeError):
        fcn(torch.zeros(2, 6, 16))
    with pytest.raises(NativeError):
        fcn_features(fcn, np.zeros((2, 6, 16)), 2)


# ------------------------------------------------------------------------------------ GPU
def _ref_op(x, w, scale, shift):
    """float64 on the CPU: TensorFlow "same" padding, conv, affine, relu; and its mean."""
    K = w.shape[2]
    pl = (K - 1) // 2
    xp = F.pad(x.double(), (pl, K - 1 - pl))
    y = F.conv1d(xp, w.double())
    y = torch.relu(y * scale.double()[None, :, None] + shift.double()[None, :, None])
    return y, y.mean(-1)


@functools.lru_cache(maxsize=None)
def _op_case(K, Ci, Co, L, B):
    g = torch.Generator().manual_seed(1000 * K + 100 * Ci + Co + L + B)
    x = torch.cumsum(0.1 * torch.randn(B, Ci, L, generator=g), -1)
    w = (torch.rand(Co, Ci, K, generator=g) * 2 - 1) / (Ci * K) ** 0.5
    scale = torch.rand(Co, generator=g) + 0.5
    shift = torch.rand(Co, generator=g) - 0.5
    return (x, w, scale, shift) + _ref_op(x, w, scale, shift)


def _close(got, ref, what):
    err, top = float((got.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: max err {err:.3e} = {err / max(top, 1e-300):.2e} of max|ref| {top:.3e}")
    assert err <= REL * top, f"{what}: {err:.3e} > {REL} * {top:.3e}"


# (K, Ci, Co, L, B): L < K; L at 63..65 and around the kernel's 128-position tile; two tiles;
# Ci K odd (5, 15, 3) and below the chunk (8, 24); the three layers' (K, Ci, Co); one and two
# 64-channel groups, and Co = 32 (half a group idle)
OP_CASES = [
    (8, 1, 32, 1, 1), (8, 3, 32, 7, 3), (8, 6, 128, 200, 3), (8, 128, 128, 65, 1),
    (5, 3, 32, 2, 3), (5, 1, 128, 63, 1), (5, 128, 256, 65, 1), (5, 6, 32, 129, 1),
    (3, 1, 32, 1, 1), (3, 128, 128, 64, 3), (3, 256, 128, 200, 1), (3, 6, 256, 128, 1),
    (1, 3, 32, 127, 3), (1, 128, 128, 2, 1), (1, 6, 256, 200, 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("K,Ci,Co,L,B", OP_CASES)
def test_conv_bn_relu_vs_float64(K, Ci, Co, L, B, cuda):
    from timevqvae.hip.fcn import conv_bn_relu
    x, w, scale, shift, yr, gr = _op_case(K, Ci, Co, L, B)
    y, gap = conv_bn_relu(x.to(cuda), w.to(cuda), scale.to(cuda), shift.to(cuda), y=True, gap=True)
    assert y.shape == (B, Co, L) and gap.shape == (B, Co)
    _close(y, yr, "y")
    _close(gap, gr, "gap")
    # the y-only launch (position tiles on the grid) writes the same values
    only, none = conv_bn_relu(x.to(cuda), w.to(cuda), scale.to(cuda), shift.to(cuda))
    assert none is None and torch.equal(only, y)


@pytest.mark.gpu
def test_padding_side_is_the_references(cuda):
    """K = 8 pads 3 on the left and 4 on the right: an impulse at position 5 under taps 1..8
    gives 8..1 at positions 1..8, exactly."""
    from timevqvae.hip.fcn import conv_bn_relu
    x = torch.zeros(1, 1, 16)
    x[0, 0, 5] = 1.0
    w = torch.arange(1.0, 9.0).repeat(32, 1, 1)
    one, zero = torch.ones(32), torch.zeros(32)
    want = torch.zeros(1, 32, 16)
    want[0, :, 1:9] = torch.arange(8.0, 0.0, -1.0)
    assert torch.equal(_ref_op(x, w, one, zero)[0].float(), want)
    y, _ = conv_bn_relu(x.to(cuda), w.to(cuda), one.to(cuda), zero.to(cuda))
    assert torch.equal(y.cpu(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("K,Ci,Co,L,B", [(8, 6, 128, 200, 3), (3, 256, 128, 200, 1),
                                         (5, 3, 32, 2, 3), (1, 3, 32, 127, 3)])
def test_gap_alone_equals_gap_with_y(K, Ci, Co, L, B, cuda):
    from timevqvae.hip.fcn import conv_bn_relu
    x, w, scale, shift, _, gr = _op_case(K, Ci, Co, L, B)
    args = [t.to(cuda) for t in (x, w, scale, shift)]
    _, both = conv_bn_relu(*args, y=True, gap=True)
    none, alone = conv_bn_relu(*args, y=False, gap=True)
    assert none is None and torch.equal(alone, both)
    _close(alone, gr, "gap")


@pytest.mark.gpu
@pytest.mark.parametrize("K,Ci,Co,L", [(8, 6, 128, 200), (5, 128, 256, 65), (3, 3, 32, 7)])
def test_rows_do_not_depend_on_the_batch(K, Ci, Co, L, cuda):
    from timevqvae.hip.fcn import conv_bn_relu
    x, w, scale, shift, _, _ = _op_case(K, Ci, Co, L, 5)
    x, w, scale, shift = (t.to(cuda) for t in (x, w, scale, shift))
    y5, g5 = conv_bn_relu(x, w, scale, shift, y=True, gap=True)
    y1, g1 = conv_bn_relu(x[2:3], w, scale, shift, y=True, gap=True)
    assert torch.equal(y5[2:3], y1) and torch.equal(g5[2:3], g1)


@pytest.mark.gpu
def test_features_do_not_depend_on_the_batch_size(cuda):
    from timevqvae.evaluation import fcn_class_probabilities, fcn_features
    fcn = _fcn(6, 5, 171, cuda)
    x = golden("g17_fcn.npz")["a_x"][:5]
    assert np.array_equal(fcn_features(fcn, x, 2), fcn_features(fcn, x, 5))
    assert np.array_equal(fcn_class_probabilities(fcn, x, 2), fcn_class_probabilities(fcn, x, 5))


@pytest.mark.gpu
def test_batch_beyond_65535_rides_the_grid(cuda):
    from timevqvae.hip.fcn import conv_bn_relu
    B = 65537
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 1, 2, generator=g).to(cuda)
    w = torch.randn(32, 1, 3, generator=g).to(cuda)
    scale, shift = torch.rand(32, generator=g).to(cuda) + 0.5, torch.rand(32, generator=g).to(cuda)
    y, gap = conv_bn_relu(x, w, scale, shift, y=True, gap=True)
    for r in (0, B - 1):
        y1, g1 = conv_bn_relu(x[r:r + 1], w, scale, shift, y=True, gap=True)
        assert torch.equal(y[r:r + 1], y1) and torch.equal(gap[r:r + 1], g1)
    assert float(y[B - 1].abs().sum()) > 0.0


@pytest.mark.gpu
def test_refusals_name_the_argument(cuda):
    from timevqvae.hip import NativeError
    from timevqvae.hip.fcn import conv_bn_relu
    x = torch.zeros(2, 3, 16, device=cuda)

    def run(Co, K, **kw):
        v = torch.ones(Co, device=cuda)
        return conv_bn_relu(x, torch.zeros(Co, 3, K, device=cuda), v, v, **kw)
    with pytest.raises(NativeError, match="Co=48"):
        run(48, 3)
    with pytest.raises(NativeError, match="K=9"):
        run(32, 9)
    with pytest.raises(NativeError, match="y and gap"):
        run(32, 3, y=False, gap=False)
    y, gap = run(32, 3, y=True, gap=True)  # legal arguments run: relu(1 * 0 + 1) everywhere
    assert float(y.min()) == 1.0 == float(y.max()) and float(gap.min()) == 1.0 == float(gap.max())


@pytest.mark.gpu
@pytest.mark.parametrize("classes", [1, 2, 37, 200])
def test_head_vs_float64(classes, cuda):
    from timevqvae.hip.fcn import head
    g = torch.Generator().manual_seed(classes)
    feat = torch.rand(5, 128, generator=g)
    w = torch.rand(classes, 128, generator=g) * 2 - 1
    b = torch.rand(classes, generator=g) - 0.5
    ref = feat.double() @ w.double().T + b.double()
    logits, probs = head(feat.to(cuda), w.to(cuda), b.to(cuda), probs=True)
    _close(logits, ref, "logits")
    perr = float((probs.double().cpu() - torch.softmax(ref, -1)).abs().max())
    serr = float((probs.double().sum(-1) - 1).abs().max())
    print(f"probs: max abs err {perr:.3e}, row sums off by {serr:.3e}")
    assert perr <= 1e-6 and serr <= 1e-6
    assert torch.equal(head(feat.to(cuda), w.to(cuda), b.to(cuda)), logits)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_network_vs_reference_golden(name, cuda):
    from timevqvae.evaluation import fcn_class_probabilities, fcn_features, fcn_inception_score
    g = golden("g17_fcn.npz")
    cin, classes, wseed, _, shape = CASES[name]
    fcn = _fcn(cin, classes, wseed, cuda)
    x = torch.from_numpy(g[f"{name}_x"]).to(cuda)
    assert tuple(x.shape) == shape
    feat, logits = fcn(x, return_feature_vector=True), fcn(x)
    _close(feat, torch.from_numpy(g[f"{name}_feat64"]), "features")
    _close(logits, torch.from_numpy(g[f"{name}_logits64"]), "logits")
    assert np.array_equal(logits.argmax(-1).cpu().numpy(), g[f"{name}_logits64"].argmax(-1))
    assert np.array_equal(fcn_features(fcn, g[f"{name}_x"], 4), feat.cpu().numpy())
    probs = fcn_class_probabilities(fcn, g[f"{name}_x"].astype(np.float64), 4)
    # |dp| <= p (1 - p) 2 max|dlogit| <= max|dlogit| / 2, the logits' bound, plus the head's 1e-6
    ptol = 0.5 * REL * float(np.abs(g[f"{name}_logits64"]).max()) + 1e-6
    assert probs.dtype == np.float32 and np.abs(probs - g[f"{name}_probs"]).max() <= ptol
    if name == "a":
        np.random.seed(0)
        got = fcn_inception_score(fcn, g["a_x"], 4, n_split=1)[0]
        want = float(g["a_is"])
        print(f"IS {got:.8f} vs reference {want:.8f}")
        assert abs(got - want) <= 1e-4 * want


@pytest.mark.gpu
def test_changed_weights_are_seen(cuda):
    """The cached fold / pack follows in-place updates of parameters and buffers."""
    x = torch.from_numpy(golden("g17_fcn.npz")["a_x"]).to(cuda)
    fcn = _fcn(6, 5, 171, cuda)
    before = fcn(x)
    assert torch.equal(fcn(x), before)  # cached path: the same result
    with torch.no_grad():
        fcn.layers[1].layers[1].running_var.mul_(2)
    after = fcn(x)
    assert not torch.equal(after, before)
    sd = fcn_state(6, 5, 171)
    sd["layers.1.layers.1.running_var"] = sd["layers.1.layers.1.running_var"] * 2
    fresh = _fcn(6, 5, 3, cuda)
    fresh(x)  # fills its cache with other weights first
    fresh.load_state_dict(sd)
    assert torch.equal(fresh(x), after)
    fcn.load_state_dict(fcn_state(6, 5, 3))
    assert torch.equal(fcn(x), _fcn(6, 5, 3, cuda)(x))


@pytest.mark.gpu
def test_fcn_features_plug_into_tau_search_and_fid(cuda):
    from test_stage3 import CFG, _stage3
    from timevqvae.evaluation import calculate_fid, fcn_features
    fcn = _fcn(6, 5, 171, cuda)
    g = torch.Generator().manual_seed(6)
    X = torch.cumsum(0.1 * torch.randn(48, 6, 128, generator=g), -1).numpy()
    st = _stage3(cuda)
    tau = st.search_optimal_tau(X, cuda, n_samples=48, batch_size=16,
                                feature_fn=lambda X: fcn_features(fcn, X, 16))
    assert tau in CFG["tau_search_rng"]
    assert all(np.isfinite(v) for v in st.tau_fids.values())
    za, zb = fcn_features(fcn, X[:24], 16), fcn_features(fcn, 1.5 * X[24:], 16)
    assert za.shape == (24, 128) and za.dtype == np.float32
    fid = float(calculate_fid(za, zb))
    assert np.isfinite(fid) and fid >= -1e-6
