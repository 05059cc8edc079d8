"""FidelityEnhancer training ops (timevqvae.hip.fe_train over csrc/tvq_fe_train.hip), op by
op: every gradient the six non-conv backward kernels return, and the GroupNorm+Snake
training forward with its saved statistics, against the same expression in torch on the
CPU (the expressions of oracle/tvq_oracle.py: fe_ws_conv's weight formula, F.group_norm +
Snake, fe_layernorm, the cores inside fe_linear_attention / fe_attention), differentiated by
autograd in float64 with the same inputs and upstream gradient.

Bound, per tensor and elementwise: |got - ref64| <= 1e-5 max|ref64| + 1e-4 |ref64| (the
forward kernels' atol 1e-5 / rtol 1e-4 of test_fidelity_enhancer.py with the absolute part
scaled by the tensor's magnitude), and rel-L2 <= 1e-5 (test_ops_gpu.py).  The attention
gradient is checked as the one dqkv tensor the op returns (at n = 1 its dq and dk thirds
are zero up to rounding, so they have no magnitude of their own).  Every case first
requires float32 CPU torch to stay within a quarter of the bound, so a badly conditioned
input fails as a test-input error and not as a kernel error.

cat_interp is compared with float32 CPU torch instead (torch computes the source index in
float as the kernel does; the float64 weights differ by up to eps * src, which is no kernel
error): each gradient element is a sum of at most m = 2 ceil(L / Lin) + 2 products with
non-negative weights, two float32 summation orders of it differ by at most
2 (m + 2) 2^-24 S_j, S_j the same backward applied to |gout|.

The launch checks of the two attention backwards (LDS) are pinned as clean argument
errors; they are host-side checks that return before any launch (tvq_fe_*_attention_bwd in
csrc/tvq_fe_train.hip: TVQ_CHECK_ARG on the LDS bytes precedes hipLaunchKernelGGL)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-5
H, DH = 4, 32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ratio(t, ref, tol):
    d = (t.double() - ref).abs()
    r = torch.where(tol > 0, d / tol.clamp_min(1e-300), torch.where(d > 0, math.inf, 0.0))
    return float(r.max())


def _check(got, ref64, ref32, what):
    """The module bound for one tensor; the float32 CPU reference must use <= 1/4 of it."""
    got = got.detach().cpu()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    tol = 1e-5 * ref64.abs().max() + 1e-4 * ref64.abs()
    r32, rk = _ratio(ref32, ref64, tol), _ratio(got, ref64, tol)
    rel = float((got.double() - ref64).norm() / (ref64.norm() + 1e-30))
    print(f"{what}: kernel {rk:.3f} / float32 torch {r32:.3f} of the bound, rel-L2 {rel:.2e}")
    assert r32 <= 0.25, f"{what}: test input: float32 torch at {r32:.3f} of the bound"
    assert rk <= 1.0, f"{what}: {rk:.3f} of the bound"
    assert rel <= 1e-5, f"{what}: rel-L2 {rel:.3e}"


def _ref(fn, inputs, gy, dtype):
    """fn's value and its gradients w.r.t. every non-None input, on the CPU in `dtype`."""
    xs = [None if t is None else t.detach().to(dtype).requires_grad_() for t in inputs]
    y = fn(*xs)
    gs = torch.autograd.grad(y, [x for x in xs if x is not None], gy.to(dtype))
    return y.detach(), gs


def _dev(fn, inputs, gy, cuda):
    xs = [None if t is None else t.detach().to(cuda).requires_grad_() for t in inputs]
    y = fn(*xs)
    gyd = gy.to(cuda)
    gs = torch.autograd.grad(y, [x for x in xs if x is not None], gyd)
    torch.cuda.synchronize()
    return y.detach(), gs, gyd


def _check_all(fn_hip, fn_ref, inputs, gy, names, cuda, fwd=False):
    y64, g64 = _ref(fn_ref, inputs, gy, torch.float64)
    y32, g32 = _ref(fn_ref, inputs, gy, torch.float32)
    yd, gd, gyd = _dev(fn_hip, inputs, gy, cuda)
    if fwd:
        _check(yd, y64, y32, "fwd")
    assert len(gd) == len(names)
    for got, r64, r32, n in zip(gd, g64, g32, names):
        _check(got, r64, r32, n)
    return yd, gd, gyd


# ---------------------------------------------------------------- weight standardisation
def _ws_ref(w):
    mean = w.mean(dim=(1, 2), keepdim=True)
    var = w.var(dim=(1, 2), unbiased=False, keepdim=True)
    return (w - mean) * (var + EPS).rsqrt()


# n = 18 < one block; 288 = a block and a remainder; 900 = several strides; 3 = the
# shortest row the Unet has (6 output channels over 1 input channel)
WS_SHAPES = [(8, 6, 3), (64, 96, 3), (16, 300, 3), (6, 1, 3)]


@pytest.mark.parametrize("O,Ci,K", WS_SHAPES)
def test_standardize_weight(O, Ci, K, cuda):
    from timevqvae.hip import fe_train
    g = _gen(O * 1000 + Ci)
    w, gy = torch.randn(O, Ci, K, generator=g), torch.randn(O, Ci, K, generator=g)
    _check_all(lambda t: fe_train.standardize_weight(t, EPS), _ws_ref, [w], gy, ["dw"], cuda)


def test_standardize_weight_accumulates(cuda):
    """accumulate = 1 adds the gradient onto a non-zero dw."""
    from timevqvae.hip._native import call, ptr, stream_ptr
    O, Ci, K = 64, 96, 3
    g = _gen(7)
    w, gy, dw0 = (torch.randn(O, Ci, K, generator=g) for _ in range(3))
    _, (r64,) = _ref(_ws_ref, [w], gy, torch.float64)
    _, (r32,) = _ref(_ws_ref, [w], gy, torch.float32)
    wd, gd, dw = w.to(cuda), gy.to(cuda), dw0.to(cuda)
    call("tvq_fe_ws_weight_bwd", ptr(wd), O, Ci * K, EPS, ptr(gd), ptr(dw), 1, stream_ptr())
    torch.cuda.synchronize()
    _check(dw, dw0.double() + r64, dw0 + r32, "dw0 + dw")


# ---------------------------------------------------------------- GroupNorm + Snake
G = 4
# 80 elements per group (< 256 threads); odd L over several strides; one channel row
# shorter than a wave; 600 and 1800 elements per group; 6 elements per group
GN_SHAPES = [(3, 8, 40), (2, 8, 301), (2, 64, 37), (2, 16, 150), (2, 96, 75), (1, 8, 3)]


def _gn_inputs(B, C, L, seed):
    g = _gen(seed)
    x = torch.randn(B, C, L, generator=g)
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    a = 0.2 + 0.3 * torch.rand(1, C, 1, generator=g)  # as SnakeActivation holds it
    res, gy = torch.randn(B, C, L, generator=g), torch.randn(B, C, L, generator=g)
    return x, gam, bet, a, res, gy


def _gn_ref(x, gam, bet, a, res=None, keep=None, scale=1.0):
    u = F.group_norm(x, G, gam, bet, EPS)
    s = u + (1 / a) * torch.sin(a * u) ** 2
    if keep is not None:
        s = s * keep.to(s.dtype) * scale
    return s + res if res is not None else s


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("B,C,L", GN_SHAPES)
def test_group_norm_snake(B, C, L, with_res, cuda):
    from timevqvae.hip import fe_train
    x, gam, bet, a, res, gy = _gn_inputs(B, C, L, B * 100000 + C * 1000 + L)
    inputs = [x, gam, bet, a, res if with_res else None]
    names = ["dx", "dgamma", "dbeta", "da"] + (["dres"] if with_res else [])
    _, gd, gyd = _check_all(
        lambda x_, g_, b_, a_, r_: fe_train.group_norm_snake(x_, G, g_, b_, a_, EPS, residual=r_),
        _gn_ref, inputs, gy, names, cuda, fwd=True)
    if with_res:
        assert torch.equal(gd[4], gyd), "the residual's gradient is the upstream gradient"


@pytest.mark.parametrize("B,C,L", GN_SHAPES)
def test_group_norm_snake_saved_statistics(B, C, L, cuda):
    """mean / rstd of each (b, g) as tvq_fe_gn_snake_train_fwd saves them for the backward."""
    from timevqvae.hip._native import call, ptr, stream_ptr
    x, gam, bet, a, _, _ = _gn_inputs(B, C, L, B * 100000 + C * 1000 + L)
    xd, gd, bd, ad = (t.to(cuda).contiguous() for t in (x, gam, bet, a.reshape(-1)))
    y, mean, rstd = torch.empty_like(xd), torch.empty(B * G, device=cuda), torch.empty(B * G, device=cuda)
    call("tvq_fe_gn_snake_train_fwd", ptr(xd), B, C, L, G, ptr(gd), ptr(bd), ptr(ad), EPS, 0.0,
         None, 0, None, ptr(y), ptr(mean), ptr(rstd), stream_ptr())
    torch.cuda.synchronize()
    x64, x32 = x.double().reshape(B * G, -1), x.reshape(B * G, -1)
    _check(mean, x64.mean(1), x32.mean(1), "mean")
    _check(rstd, (x64.var(1, unbiased=False) + EPS).rsqrt(),
           (x32.var(1, unbiased=False) + EPS).rsqrt(), "rstd")
    _check(y, _gn_ref(*(t.double() for t in (x, gam, bet, a))), _gn_ref(x, gam, bet, a), "fwd")


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
def test_group_norm_snake_dropout(with_res, cuda):
    """p = 0.5 at 600 elements per group and 8 (b, g) blocks (the mask index base + i beyond
    the first block): the mask is read from the output, and every gradient is that of the
    same masked expression."""
    from timevqvae.hip import fe_train, rng
    B, C, L = 2, 16, 150
    x, gam, bet, a, res, gy = _gn_inputs(B, C, L, 5)
    site = rng.new_site()
    xd, gd_, bd, ad = (t.to(cuda) for t in (x, gam, bet, a))
    y0 = fe_train.group_norm_snake(xd, G, gd_, bd, ad, EPS, drop_p=0.0)
    calls = rng._calls[0]
    y = fe_train.group_norm_snake(xd, G, gd_, bd, ad, EPS, drop_p=0.5, site=site)
    keep = y != 0
    assert 0.3 < keep.float().mean().item() < 0.7
    torch.testing.assert_close(y[keep], 2 * y0[keep], rtol=1e-6, atol=1e-6)
    for b in range(B):  # every (b, g) block has its own draws
        for g_ in range(G):
            blk = keep[b, g_ * (C // G):(g_ + 1) * (C // G)]
            assert 0.3 < blk.float().mean().item() < 0.7, (b, g_)
    assert not torch.equal(keep[0], keep[1])
    keep_c = keep.cpu()
    rng._calls[0] = calls  # the same draws again
    inputs = [x, gam, bet, a, res if with_res else None]
    names = ["dx", "dgamma", "dbeta", "da"] + (["dres"] if with_res else [])
    yd, gd, gyd = _check_all(
        lambda x_, g_, b_, a_, r_: fe_train.group_norm_snake(x_, G, g_, b_, a_, EPS, residual=r_,
                                                            drop_p=0.5, site=site),
        lambda x_, g_, b_, a_, r_: _gn_ref(x_, g_, b_, a_, r_, keep_c, 2.0),
        inputs, gy, names, cuda, fwd=True)
    if with_res:
        assert torch.equal(gd[4], gyd)
    else:
        assert torch.equal(yd != 0, keep)


# ---------------------------------------------------------------- channel LayerNorm
def _ln_ref(x, g, res=None):
    var = torch.var(x, dim=1, unbiased=False, keepdim=True)
    mean = torch.mean(x, dim=1, keepdim=True)
    y = (x - mean) * (var + EPS).rsqrt() * g
    return y + res if res is not None else y


# B L = 602 (no multiple of 256); L shorter than a wave; L = 1; one image, C = 128
LN_SHAPES = [(2, 8, 301), (3, 64, 37), (300, 16, 1), (1, 128, 5)]


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("B,C,L", LN_SHAPES)
def test_channel_layernorm(B, C, L, with_res, cuda):
    from timevqvae.hip import fe_train
    g = _gen(B * 100000 + C * 1000 + L)
    x, gain = torch.randn(B, C, L, generator=g), torch.randn(1, C, 1, generator=g)
    res, gy = torch.randn(B, C, L, generator=g), torch.randn(B, C, L, generator=g)
    inputs = [x, gain, res if with_res else None]
    names = ["dx", "dg"] + (["dres"] if with_res else [])
    _, gd, gyd = _check_all(lambda x_, g_, r_: fe_train.channel_layernorm(x_, g_, EPS, residual=r_),
                            _ln_ref, inputs, gy, names, cuda)
    if with_res:
        assert torch.equal(gd[2], gyd)


# ---------------------------------------------------------------- attention cores
def _linattn_ref(qkv):
    b, _, n = qkv.shape
    q, k, v = (t.reshape(b, H, DH, n) for t in qkv.chunk(3, dim=1))
    q = q.softmax(dim=-2) * DH ** -0.5
    k = k.softmax(dim=-1)
    context = torch.einsum("bhdn,bhen->bhde", k, v)
    return torch.einsum("bhde,bhdn->bhen", context, q).reshape(b, H * DH, n)


def _attn_ref(qkv):
    b, _, n = qkv.shape
    q, k, v = (t.reshape(b, H, DH, n) for t in qkv.chunk(3, dim=1))
    attn = torch.einsum("bhdi,bhdj->bhij", q * DH ** -0.5, k).softmax(dim=-1)
    out = torch.einsum("bhij,bhdj->bhid", attn, v)
    return out.permute(0, 1, 3, 2).reshape(b, H * DH, n)


def _attn_case(fn_hip, fn_ref, n, scale, cuda):
    B = 2
    g = _gen(n * 10 + int(scale))
    qkv = scale * torch.randn(B, 3 * H * DH, n, generator=g)
    gy = torch.randn(B, H * DH, n, generator=g)
    (_, (r64,)), (_, (r32,)) = (_ref(fn_ref, [qkv], gy, dt) for dt in (torch.float64, torch.float32))
    _, (got,), _ = _dev(lambda t: fn_hip(t, H, DH), [qkv], gy, cuda)
    _check(got, r64, r32, "dqkv")


# one key; below / at / above a wave (the k softmax and the dk dot stride by 64 lanes);
# more than one stride of the block's 256 threads; n = 403, the largest the launch check
# admits; the same with peaked softmaxes (inputs scaled by 4)
@pytest.mark.parametrize("n,scale", [(1, 1.0), (37, 1.0), (63, 1.0), (64, 1.0), (65, 1.0), (256, 1.0),
                                     (301, 1.0), (403, 1.0), (403, 4.0)])
def test_linear_attention(n, scale, cuda):
    from timevqvae.hip import fe_train
    _attn_case(fe_train.linear_attention, _linattn_ref, n, scale, cuda)


# one key; a row loop shorter / longer than a wave; n = 112, the largest admitted; the same
# with peaked softmaxes (inputs scaled by 4)
@pytest.mark.parametrize("n,scale", [(1, 1.0), (31, 1.0), (37, 1.0), (64, 1.0), (65, 1.0), (112, 1.0),
                                     (112, 4.0)])
def test_attention(n, scale, cuda):
    from timevqvae.hip import fe_train
    _attn_case(fe_train.attention, _attn_ref, n, scale, cuda)


def _attn_bwd_call(op, n, cuda):
    """The backward entry point on valid buffers of the right size (whatever it decides)."""
    from timevqvae.hip._native import call, ptr, stream_ptr
    B = 2
    g = _gen(n)
    qkv = torch.randn(B, 3 * H * DH, n, generator=g).to(cuda)
    gy = torch.randn(B, H * DH, n, generator=g).to(cuda)
    dqkv = torch.zeros_like(qkv)
    call(op, ptr(qkv), ptr(gy), B, H, DH, n, ptr(dqkv), stream_ptr())
    torch.cuda.synchronize()
    return dqkv


@pytest.mark.parametrize("op,n_bad,n_ok", [("tvq_fe_linear_attention_bwd", 404, 403),
                                           ("tvq_fe_attention_bwd", 113, 112)])
def test_attention_backward_limits(op, n_bad, n_ok, cuda):
    """Past its limit (include/tvq.h: linear attention n <= 403, full attention n <= 112) the
    backward is a clean TVQ_ERR_ARG naming the op, returned by the host-side check before any
    launch, and the next call at a supported n succeeds."""
    from timevqvae.hip._native import NativeError, lib
    with pytest.raises(NativeError, match=rf"{op} failed \(-1\)"):
        _attn_bwd_call(op, n_bad, cuda)
    assert op in lib().tvq_last_error().decode()
    assert torch.isfinite(_attn_bwd_call(op, n_ok, cuda)).all()


# ---------------------------------------------------------------- interpolate + concat
def _interp(t, L):
    return F.interpolate(t, size=L, mode="linear", align_corners=False)


def _cat_ref(a, b, L):
    return _interp(a, L) if b is None else torch.cat((_interp(a, L), _interp(b, L)), 1)


# up and down by ragged ratios, identity on one side, a 30:1 and a 1:3.3 ratio, equal
# lengths throughout, a single input sample; b = None (the input / output interpolation)
@pytest.mark.parametrize("La,Lb,L", [(17, 40, 33), (301, 150, 301), (37, 75, 75), (300, 10, 33),
                                     (5, 5, 5), (1, 2, 7), (256, None, 301), (301, None, 301)])
def test_cat_interp(La, Lb, L, cuda):
    from timevqvae.hip import fe_train
    B, Ca, Cb = 2, 3, 5
    g = _gen(La * 1000 + L)
    a = torch.randn(B, Ca, La, generator=g)
    b = torch.randn(B, Cb, Lb, generator=g) if Lb else None
    gy = torch.randn(B, Ca + (Cb if Lb else 0), L, generator=g)
    inputs = [a, b]
    _, want = _ref(lambda a_, b_: _cat_ref(a_, b_, L), inputs, gy, torch.float32)
    _, S = _ref(lambda a_, b_: _cat_ref(a_, b_, L), inputs, gy.abs(), torch.float32)
    _, got, _ = _dev(lambda a_, b_: fe_train.cat_interp(a_, b_, L), inputs, gy, cuda)
    assert len(got) == len(want)
    for name, Lin, d, w, s in zip(("da", "db"), (La, Lb), got, want, S):
        m = 2 * math.ceil(L / Lin) + 2
        tol = 2 * (m + 2) * 2.0 ** -24 * s.double()
        d = d.cpu()
        assert d.shape == w.shape
        r = _ratio(d, w.double(), tol)
        print(f"{name} ({Lin} -> {L}): {r:.3f} of the summation-order bound")
        assert r <= 1.0, f"{name}: {r:.3f} of the bound"
