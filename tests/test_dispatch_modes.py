"""The Python gates in front of the fused kernels, off the diagonal the benchmark runs on.

Every fused kernel has a per-op fallback and a predicate that chooses between them
(resblock.supported / proj_supported / pair_supported, bnstats_blocks, bn_eval_fusable,
fused_ff_supported, attn_branch_supported, tied_ce_supported, hf_embed_supported,
upscale.supported, and the `self.training` / `bn.training` branches of models/vq_vae.py and
models/bidirectional_transformer.py).  The kernels' own tests run them in one module state:
the whole tree in train() or in eval(), every parameter trainable, pointers 16-byte aligned.
This module pins what the gates decide elsewhere:

  1. block mode x BatchNorm mode x grad mode for the conv + BN blocks (a frozen BatchNorm
     inside a training block keeps its statistics and normalises with them);
  2. frozen parameters, FusedAdamW's flat gradients with a frozen parameter, an input without
     gradient, and gradient accumulation through every fused autograd.Function;
  3. parameters that are not 16-byte aligned (packed after an odd-sized one in FusedAdamW's
     flat buffer), the bias shapes of the tied cross-entropy, non-contiguous inputs.

The reference in every part is plain torch on the CPU in float64 (F.conv2d / F.batch_norm,
which honours the BatchNorm's own mode / the Snake formula / softmax), never the project's
other path alone.  Where a case is meant to run a fused kernel, the plan trace is asserted,
so that the fallback is not compared with itself.

Bars (taken from the tests of the same ops, not from what the code gives): conv + BN units:
output 1e-4 of the reference's max-abs, running statistics 1e-5 (test_bn_stats.py), gradients
rel-L2 1e-5, input and Snake `a` gradients rel-L2 2e-5 (test_ops_gpu.py); a conv bias ahead of
a training BatchNorm has a true gradient of 0 and is held to 2e-5 of its conv's weight
gradient (test_resblock.py).  Attention / feed-forward: rel-L2 1e-5 (test_fused_attn.py,
test_fused_ff.py).  Tied cross-entropy: loss 1e-5, gradients 1e-4 of max-abs
(test_tied_ce.py).  hf_embed_folded: 1e-5 / 2e-5, weight_product: 1e-5 of max-abs
(test_hf_embed_fold.py).
"""
import copy
import functools
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

gpu = pytest.mark.gpu


def rel_max(a, r):
    a, r = a.detach().double().cpu(), r.detach().double().cpu()
    return float((a - r).abs().max() / r.abs().max().clamp_min(1e-30))


def rel_l2(a, r):
    a, r = a.detach().double().cpu(), r.detach().double().cpu()
    return float((a - r).norm() / (r.norm() + 1e-30))


# --------------------------------------------------------------------- fp64 references
def snake64(u, a):
    return u + (1.0 / a) * torch.sin(a * u) ** 2


class Ref:
    """float64 leaf copies of a module's parameters and buffers; `bn` is F.batch_norm in the
    mode of the BatchNorm module it restates, updating the copied buffers as torch does."""

    def __init__(self, m):
        self.P = {k: v.detach().double().clone().requires_grad_(True)
                  for k, v in m.named_parameters()}
        self.B = {k: (v.detach().double().clone() if v.is_floating_point() else v.detach().clone())
                  for k, v in m.named_buffers()}

    def bn(self, h, pre, mod):
        y = F.batch_norm(h, self.B[pre + "running_mean"], self.B[pre + "running_var"],
                         self.P[pre + "weight"], self.P[pre + "bias"], mod.training, mod.momentum,
                         mod.eps)
        if mod.training:
            self.B[pre + "num_batches_tracked"] += 1
        return y


def ref_enc(R, m, x):
    P = R.P
    h = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), P["block.0.weight"], P["block.0.bias"],
                 stride=(1, 2))
    return snake64(R.bn(h, "block.1.", m.block[1]), P["block.2.a"])


def ref_dec(R, m, x):
    P = R.P
    h = F.conv_transpose2d(x, P["block.0.weight"], P["block.0.bias"], stride=(1, 2), padding=(1, 1))
    return snake64(R.bn(h, "block.1.", m.block[1]), P["block.2.a"])


def ref_res(R, m, x, pre=""):
    P = R.P
    s = snake64(x, P[pre + "convs.0.a"])
    h = F.conv2d(s, P[pre + "convs.1.weight"], P[pre + "convs.1.bias"], padding=1)
    v = snake64(R.bn(h, pre + "convs.2.", m.convs[2]), P[pre + "convs.3.a"])
    o = F.conv2d(v, P[pre + "convs.4.weight"], P[pre + "convs.4.bias"], padding=1)
    if isinstance(m.proj, nn.Identity):
        return x + o
    return F.conv2d(x, P[pre + "proj.weight"], P[pre + "proj.bias"]) + o


def ref_pair(R, m, x):
    return ref_res(R, m[1], ref_res(R, m[0], x, "0."), "1.")


UPS_M = 96


def ref_ups(R, m, x):
    P = R.P
    u = F.interpolate(x.transpose(1, 2), size=UPS_M, mode="nearest")
    h = F.gelu(F.conv1d(u, P["conv.0.weight"], P["conv.0.bias"], padding=1))
    return R.bn(h, "conv.2.", m.conv[2])


def ref_bnsnake(R, m, x):
    return snake64(R.bn(x, "bn.", m.bn), R.P["a"])


def ref_attn(R, m, x):
    P = R.P
    B, S, D = x.shape
    xn = F.normalize(x, dim=-1) * math.sqrt(D) * P["norm.g"]
    q, k, v = (F.linear(xn, P[f"attn.to_{c}.weight"]).view(B, S, 2, 64).transpose(1, 2)
               for c in "qkv")
    o = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v
    return x + F.linear(o.transpose(1, 2).reshape(B, S, D), P["attn.to_out.weight"])


def ref_ff(R, m, x, r):
    P = R.P
    h = F.gelu(F.linear(x, P["ff.ff.0.0.weight"], P["ff.ff.0.0.bias"]))
    return r + F.linear(h, P["ff.ff.2.weight"], P["ff.ff.2.bias"])


TCE_K = 64


def ref_tiedce(R, m, h, tgt, keep):
    P = R.P
    logits = h @ P["W"][:TCE_K].t() + P["bias"][:, :TCE_K]  # torch's own broadcast rules
    return F.cross_entropy(logits[~keep], tgt[~keep])


def ref_hfembed(R, m, x, th, cls):
    P = R.P
    mm = x.shape[2]
    up = F.conv1d(x, P["W2"], P["b2"], padding=1).transpose(1, 2)
    emb = torch.cat([cls, torch.cat([up, th], -1) + P["pos"][:mm]], 1)
    return emb @ P["W_in"].t()


def ref_wprod(R, m):
    return R.P["w1"] @ R.P["w2"]


# --------------------------------------------------------------------- the device side
def fwd_call(m, x):
    return m(x)


def fwd_pair(m, x):
    from timevqvae.models.vq_vae import run_layers
    return run_layers(m, x, lambda layer, v: layer(v))


def fwd_ups(m, x):
    return m.first(x, UPS_M)


def fwd_bnsnake(m, x):
    from timevqvae.hip.norm import bn_snake
    return bn_snake(x, m.bn, m.a)


def fwd_attn(m, x):
    """The attention layer as Encoder.forward dispatches it."""
    from timevqvae.hip import xf
    if xf.attn_branch_supported(x, m.norm.g, m.attn):
        return xf.attn_branch(x, m.norm.g, m.attn, None, 0.0)
    n, r = xf.rmsnorm_res(x, m.norm.g)
    return m.attn(n, residual=r, gate=None)


def fwd_ff(m, x, r):
    return m.ff(x, residual=r, gate=None)


def fwd_tiedce(m, h, tgt, keep):
    from timevqvae.models.bidirectional_transformer import tied_logits_ce
    m._one = torch.ones((), device=h.device)  # the root gradient of forward_backward
    return tied_logits_ce(h, m.W, m.bias, TCE_K, tgt, keep, m._one)


def fwd_hfembed(m, x, th, cls):
    from timevqvae.hip.upscale import hf_embed_folded, hf_embed_supported
    assert hf_embed_supported(x, th, m.W_in, m.W2, m.pos)
    return hf_embed_folded(x, th, cls, m.W_in, m.W2, m.b2, m.pos)


def fwd_wprod(m):
    from timevqvae.hip.linear import weight_product
    return weight_product(m.w1, m.w2)


class Holder(nn.Module):
    """Parameters / sub-modules of a functional unit under one module (named, movable,
    copyable, visible to FusedAdamW)."""

    def __init__(self, **kw):
        super().__init__()
        for k, v in kw.items():
            setattr(self, k, nn.Parameter(v) if isinstance(v, torch.Tensor) else v)


def _init(m):
    """Convs / Linears ~ N(0, 1.5^2 / fan_in); BatchNorm as test_bn_stats._block: weight
    N(1, 0.3), bias N(0, 0.3), running_mean N(0, 1), running_var U(0.5, 2); Snake a U(0.3, 0.8)."""
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (nn.modules.conv._ConvNd, nn.Linear)):
                fan = mod.weight[0].numel() if not isinstance(mod, nn.ConvTranspose2d) \
                    else mod.weight[:, 0].numel()
                mod.weight.normal_(0.0, 1.5 / math.sqrt(fan))
                if mod.bias is not None:
                    mod.bias.normal_(0.0, 0.5)
            elif isinstance(mod, nn.modules.batchnorm._BatchNorm):
                mod.weight.normal_(1.0, 0.3)
                mod.bias.normal_(0.0, 0.3)
                mod.running_mean.normal_()
                mod.running_var.uniform_(0.5, 2.0)
        for k, p in m.named_parameters():
            if k == "a" or k.endswith(".a"):
                p.uniform_(0.3, 0.8)
            elif k.endswith(".g"):
                p.uniform_(0.5, 1.5)
    return m


def mk_enc():
    from timevqvae.models.vq_vae import VQVAEEncBlock
    return VQVAEEncBlock(4, 8, False)


def mk_dec():
    from timevqvae.models.vq_vae import VQVAEDecBlock
    return VQVAEDecBlock(8, 4, False)


def mk_res(ci, co, p=0.0):
    from timevqvae.models.vq_vae import ResBlock
    return ResBlock(ci, co, False, dropout=p)


def mk_ups():
    from timevqvae.models.bidirectional_transformer import Upscale
    return Upscale(128, 128, 256)


def mk_attn():
    from timevqvae.models.bidirectional_transformer import Attention, RMSNorm
    return Holder(norm=RMSNorm(128), attn=Attention(128, 2, 64, 0.0))


def mk_ff():
    from timevqvae.models.bidirectional_transformer import FeedForward
    return Holder(ff=FeedForward(128, 1, 0.0))


def _randn(*shape, scale=1.0):
    return torch.randn(*shape) * scale


def mk_tiedce(rows=24):
    return Holder(W=_randn(TCE_K + 1, 128, scale=3 / 128 ** 0.5), bias=_randn(rows, TCE_K + 1, scale=0.2))


def mk_hfembed():
    D, H, d = 128, 256, 32
    return Holder(W_in=_randn(d, 2 * D, scale=(2 * D) ** -0.5), W2=_randn(D, H, 3, scale=(3 * H) ** -0.5),
                  b2=_randn(D, scale=0.1), pos=_randn(97, 2 * D))


def in_x(*shape):
    return lambda g: [torch.randn(*shape, generator=g) * 1.3]


def in_tiedce(g):
    keep = torch.rand(3, 24, generator=g) >= 0.36
    keep[0, 0] = False  # at least one masked token
    return [torch.randn(3, 24, 128, generator=g), torch.randint(0, TCE_K, (3, 24), generator=g), keep]


class Spec:
    def __init__(self, make, inputs, fwd, ref, bns=lambda m: [], train=(), bn_marks=(), evalm=(),
                 zero_bias=None, freeze=(), ytol=("max", 1e-4), ptol=("l2", 1e-5),
                 xtol=("l2", 2e-5)):
        self.make, self.inputs, self.fwd, self.ref, self.bns = make, inputs, fwd, ref, bns
        self.train = train        # trace substrings of the fused training path (default state)
        self.bn_marks = bn_marks  # those of them that need the BatchNorm itself to train
        self.evalm = evalm        # trace substrings of the fused eval launch (eval, no grad)
        self.zero_bias = zero_bias or {}  # conv bias ahead of a BatchNorm -> that conv's weight
        self.freeze = freeze
        self.ytol, self.ptol, self.xtol = ytol, ptol, xtol


STRIDED = dict(bns=lambda m: [m.block[1]], train=("bnstats", "bn_apply_part"),
               bn_marks=("bnstats", "bn_apply_part"), zero_bias={"block.0.bias": "block.0.weight"})
RES = dict(bns=lambda m: [m.convs[2]], zero_bias={"convs.1.bias": "convs.1.weight"})
XF = dict(ytol=("l2", 1e-5), ptol=("l2", 1e-5), xtol=("l2", 1e-5))

SPECS = {
    # output 65 wide: crosses a 64-wide segment, ragged
    "enc": Spec(mk_enc, in_x(3, 4, 3, 130), fwd_call, ref_enc, evalm=("conv_bn_eval",), **STRIDED),
    "dec": Spec(mk_dec, in_x(3, 8, 3, 40), fwd_call, ref_dec, evalm=("convT_bn_eval",), **STRIDED),
    "res16": Spec(lambda: mk_res(16, 16), in_x(3, 16, 3, 32), fwd_call, ref_res,
                  train=("rb_fwd1", "rb_bwd1"), bn_marks=("rb_fwd1", "rb_bwd1"), evalm=("rb_eval",),
                  freeze=("convs.1.weight", "convs.4.bias", "convs.3.a"), **RES),
    "res64": Spec(lambda: mk_res(64, 64), in_x(3, 64, 3, 8), fwd_call, ref_res,
                  train=("w8_fwd1", "w8_bwd1"), bn_marks=("w8_fwd1", "w8_bwd1"), evalm=("w8_eval",),
                  freeze=("convs.4.weight", "convs.2.bias", "convs.0.a"), **RES),
    "proj": Spec(lambda: mk_res(64, 128), in_x(3, 64, 3, 8), fwd_call, ref_res,
                 train=("w8p_fwd", "w8p_bwd"), bn_marks=("w8p_fwd", "w8p_bwd"), evalm=("w8p_eval",),
                 freeze=("proj.weight", "convs.4.bias", "convs.2.weight"), **RES),
    "ups": Spec(mk_ups, lambda g: [torch.randn(3, 24, 128, generator=g) * 1.3], fwd_ups, ref_ups,
                bns=lambda m: [m.conv[2]], train=("ups_combine", "ups_sums"), evalm=("mode2",)),
    "pair": Spec(lambda: nn.Sequential(mk_res(16, 16), mk_res(16, 16)), in_x(3, 16, 3, 32), fwd_pair,
                 ref_pair, bns=lambda m: [m[0].convs[2], m[1].convs[2]],
                 train=("rb_fwd21", "rb_bwd12"), bn_marks=("rb_fwd21", "rb_bwd12", "rb_fwd1"),
                 evalm=("rb_eval",),
                 zero_bias={"0.convs.1.bias": "0.convs.1.weight", "1.convs.1.bias": "1.convs.1.weight"}),
    "bnsnake": Spec(lambda: Holder(bn=nn.BatchNorm2d(16), a=torch.ones(1, 16, 1, 1)),
                    in_x(3, 16, 3, 32), fwd_bnsnake, ref_bnsnake, bns=lambda m: [m.bn],
                    freeze=("bn.weight", "bn.bias", "a")),
    "attn": Spec(mk_attn, lambda g: [torch.randn(3, 13, 128, generator=g)], fwd_attn, ref_attn,
                 train=("attn_branch_fwd", "attn_branch_bwd"),
                 freeze=("attn.to_q.weight", "attn.to_out.weight", "norm.g"), **XF),
    "ff": Spec(mk_ff, lambda g: [torch.randn(3, 13, 128, generator=g) for _ in range(2)], fwd_ff,
               ref_ff, train=("ffn_fwd", "ffn_bwd"), freeze=("ff.ff.0.0.weight", "ff.ff.2.bias"), **XF),
    "tiedce": Spec(mk_tiedce, in_tiedce, fwd_tiedce, ref_tiedce, train=("tied_logits_ce",),
                   freeze=("W", "bias"), ytol=("max", 1e-5), ptol=("max", 1e-4), xtol=("max", 1e-4)),
    "hfembed": Spec(mk_hfembed, lambda g: [torch.randn(3, 256, 96, generator=g),
                                           torch.randn(3, 96, 128, generator=g),
                                           torch.randn(3, 1, 256, generator=g)],
                    fwd_hfembed, ref_hfembed, freeze=("W_in", "b2", "pos"), ytol=("max", 1e-5),
                    ptol=("max", 2e-5), xtol=("max", 2e-5)),
    "wprod": Spec(lambda: Holder(w1=_randn(128, 256), w2=_randn(256, 32)), lambda g: [], fwd_wprod,
                  ref_wprod, freeze=("w1", "w2"), ytol=("max", 1e-5), ptol=("max", 1e-5)),
}
PART1 = ["enc", "dec", "res16", "res64", "proj", "ups", "pair"]
PART2 = ["res16", "res64", "proj", "bnsnake", "attn", "ff", "tiedce", "hfembed", "wprod"]


@functools.lru_cache(maxsize=None)
def master(name):
    """The unit's fp32 CPU module, built once; every run works on a deep copy."""
    torch.manual_seed(sum(map(ord, name)))
    return _init(SPECS[name].make())


@functools.lru_cache(maxsize=None)
def inputs(name, seed=0):
    return SPECS[name].inputs(torch.Generator().manual_seed(1000 + seed))


def set_modes(spec, m, block_train, bn_train):
    m.train(block_train)
    for bn in spec.bns(m):
        bn.train(bn_train)
    return m


@functools.lru_cache(maxsize=None)
def reference(name, bn_train=True, seed=0):
    """fp64 forward + backward of the unit on inputs(name, seed), its BatchNorms in
    `bn_train` mode -> {"y", "gy", "g": {param / "in<i>": grad}, "B": buffers afterwards}.
    Computed once per (unit, mode, seed) and shared; callers must not modify it."""
    spec = SPECS[name]
    m = set_modes(spec, copy.deepcopy(master(name)), True, bn_train)
    R = Ref(m)
    xs = [t.double().requires_grad_(True) if t.is_floating_point() else t for t in inputs(name, seed)]
    y = spec.ref(R, m, *xs)
    if y.dim() == 0:
        gy = torch.ones((), dtype=torch.float64)
    else:
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(77 + seed)).double()
    y.backward(gy)
    g = {k: p.grad for k, p in R.P.items()}
    g.update({f"in{i}": t.grad for i, t in enumerate(xs) if t.is_floating_point()})
    return {"y": y.detach(), "gy": gy, "g": g, "B": R.B}


def run(name, cuda, block_train=True, bn_train=True, grad=True, x_grad=True, m=None, seeds=(0,),
        wrap=None):
    """The unit on the device: a deep copy of the master (or `m`, already on the device) in
    the given modes, one forward (+ backward) per seed without zeroing in between."""
    from timevqvae.hip._native import plan_trace
    spec = SPECS[name]
    if m is None:
        m = copy.deepcopy(master(name)).to(cuda)
    set_modes(spec, m, block_train, bn_train)
    before = {k: v.clone() for k, v in m.named_buffers()}
    ys, xs_all, args_all = [], [], []
    with plan_trace() as tr, (torch.enable_grad() if grad else torch.no_grad()):
        for seed in seeds:
            xs = [t.to(cuda) for t in inputs(name, seed)]
            leaves = [t.requires_grad_(True) if grad and x_grad and t.is_floating_point() else t
                      for t in xs]
            args = [wrap(t) if wrap is not None and t.is_floating_point() else t for t in leaves]
            if wrap is not None:  # the wrapped inputs' leaves carry the gradients
                leaves = [getattr(a, "_leaf", a) for a in args]
            y = spec.fwd(m, *args)
            if grad:
                root = getattr(m, "_one", None) if y.dim() == 0 else None
                gy = root if root is not None else \
                    reference(name, bn_train, seed)["gy"].float().to(cuda)
                torch.autograd.backward(y, gy)
            ys.append(y.detach())
            xs_all.append(leaves)
            args_all.append(args)
        torch.cuda.synchronize()
    g = {k: p.grad for k, p in m.named_parameters()}
    for i, t in enumerate(xs_all[-1]):
        if t.is_floating_point():
            g[f"in{i}"] = t.grad
    return {"y": ys[-1], "g": g, "B": dict(m.named_buffers()), "before": before, "trace": tr.lines,
            "m": m, "leaves": xs_all, "args": args_all}


def err(kind, a, r):
    return rel_max(a, r) if kind == "max" else rel_l2(a, r)


def check_y(spec, got, ref):
    e = err(spec.ytol[0], got["y"], ref["y"])
    assert e < spec.ytol[1], ("y", e)


def check_grads(spec, got, want, bn_train=True, skip=()):
    """got: name -> device gradient; want: name -> fp64 gradient (summed over the passes)."""
    for k, r in want.items():
        if k in skip or r is None:
            continue
        g = got[k]
        assert g is not None, k
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if bn_train and k in spec.zero_bias:
            # ahead of a training BatchNorm the bias' true gradient is 0: rounding residue of
            # sums whose terms are those of the conv's weight gradient
            bound = 2e-5 * float(want[spec.zero_bias[k]].abs().max())
            e = float((g.detach().double().cpu() - r).abs().max())
            assert e <= bound, (k, e, bound)
            continue
        kind, tol = spec.xtol if (k.startswith("in") or k == "a" or k.endswith(".a")) else spec.ptol
        e = err(kind, g, r)
        assert e < tol, (k, e, tol)


def has(trace, mark):
    return any(mark in t for t in trace)


# ============================================================ 1. module-mode matrix
# (block.training, bn.training, grad enabled)
STATES = {"train_bntrain": (True, True, True), "train_bneval": (True, False, True),
          "eval_bntrain": (False, True, True), "eval_bneval_grad": (False, False, True),
          "eval_bneval_nograd": (False, False, False)}


@pytest.mark.parametrize("name", PART1)
def test_reference_separates_bn_modes(name):
    """On the fp64 reference alone (no device): BatchNorm in eval mode and in train mode give
    outputs at least 1e-2 of the output's max-abs apart, so a path that normalises with the
    wrong statistics cannot sit inside the 1e-4 output bar."""
    a, b = reference(name, True)["y"], reference(name, False)["y"]
    gap = float((a - b).abs().max() / torch.maximum(a.abs().max(), b.abs().max()))
    assert gap >= 1e-2, gap
    assert all(torch.equal(v, reference(name, False)["B"][k])  # eval: nothing moves
               for k, v in Ref(master(name)).B.items())


@gpu
@pytest.mark.parametrize("state", list(STATES))
@pytest.mark.parametrize("name", PART1)
def test_mode_matrix(name, state, cuda):
    """Output, every gradient, the running statistics and num_batches_tracked of each conv +
    BN block against torch fp64 whose BatchNorm is in the BatchNorm's own mode, in every
    combination of block mode, BatchNorm mode and grad mode; the default states take the
    fused launches (plan trace), a frozen BatchNorm takes none that computes statistics."""
    spec = SPECS[name]
    block_train, bn_train, grad = STATES[state]
    ref = reference(name, bn_train)
    got = run(name, cuda, block_train, bn_train, grad)
    tr = got["trace"]
    if bn_train:  # the gates go by the BatchNorm's own mode
        assert all(has(tr, k) for k in spec.train), tr
    if not bn_train:
        assert not any(has(tr, k) for k in spec.bn_marks), tr
    if state == "eval_bneval_nograd":
        assert all(has(tr, k) for k in spec.evalm), tr
    check_y(spec, got, ref)
    if grad:
        check_grads(spec, got["g"], ref["g"], bn_train)
    for k, r in ref["B"].items():
        b = got["B"][k]
        if not r.is_floating_point():
            assert int(b) == int(r), (k, int(b), int(r))  # num_batches_tracked
            continue
        if not bn_train:
            assert torch.equal(b, got["before"][k]), k  # bit for bit unchanged
        assert rel_max(b, r) < 1e-5, (k, rel_max(b, r))


@gpu
@pytest.mark.parametrize("name", ["res16", "res64", "proj", "pair"])
def test_frozen_bn_with_dropout(name, cuda):
    """p = 0.3 in a training block whose BatchNorm is frozen: equal to the per-op path from
    the same device seed (the pattern of test_resblock.py), the running statistics untouched,
    and against fp64: every element of the block's branch is either dropped (exactly the
    skip path) or the p = 0 reference's branch / (1 - p)."""
    from timevqvae.hip import resblock, rng
    spec = SPECS[name]
    p = 0.3
    runs = []
    for fused in (True, False):
        m = copy.deepcopy(master(name)).to(cuda)
        for mod in m.modules():
            if isinstance(mod, nn.Dropout):
                mod.p = p
        rng.manual_seed(9)
        resblock.ENABLED = fused
        try:
            runs.append(run(name, cuda, True, False, True, m=m))
        finally:
            resblock.ENABLED = True
    a, b = runs
    assert torch.equal(a["y"], b["y"])
    for k in b["g"]:
        assert torch.equal(a["g"][k], b["g"][k]), k
    for k, v in a["before"].items():
        assert torch.equal(a["B"][k], v), k
    if name == "pair":
        return  # two dropouts in a row: no element-wise fp64 statement
    ref = reference(name, False)
    x = inputs(name)[0].double()
    R = Ref(master(name))
    skip = x if name != "proj" else F.conv2d(x, R.P["proj.weight"], R.P["proj.bias"]).detach()
    want = ref["y"] - skip
    branch = a["y"].double().cpu() - skip
    tol = 1e-4 * float(ref["y"].abs().max())
    dropped = branch.abs() <= tol
    kept = (branch * (1 - p) - want).abs() <= tol
    assert bool((dropped | kept).all()), int((~(dropped | kept)).sum())
    frac = float((dropped & ~kept).float().mean())
    assert 0.2 < frac < 0.4, frac


@gpu
@pytest.mark.parametrize("name", ["enc", "dec"])
def test_strided_block_dropout_is_refused(name, cuda):
    """The Enc/DecBlocks have no dropout kernel: p > 0 in training raises, whatever the
    BatchNorm's mode (never a silent p = 0)."""
    m = copy.deepcopy(master(name)).to(cuda)
    m.block[3].p = 0.3
    with pytest.raises(NotImplementedError):
        run(name, cuda, True, False, True, m=m)


# ============================================================ 2. frozen parameters, flat gradients
def _param(m, key):
    return dict(m.named_parameters())[key]


SENTINEL = -123.456

FROZEN_CASES = [(n, k, mode) for n in PART2 for k in SPECS[n].freeze
                for mode in ("plain", "flat_pre", "flat_post")]


@gpu
@pytest.mark.parametrize("name,key,mode", FROZEN_CASES)
def test_frozen_parameter(name, key, mode, cuda):
    """One parameter frozen: plain parameters (state 1), FusedAdamW built with it already
    frozen so that it is no part of the flat buffer (2), FusedAdamW built first and the
    parameter frozen afterwards, flat but not trainable (3).  Every other gradient and dx
    match fp64; the frozen one's .grad stays None (1, 2) or, in the flat buffer, bit for bit
    the sentinel it held (3)."""
    from timevqvae.hip.optim import FusedAdamW
    spec = SPECS[name]
    m = copy.deepcopy(master(name)).to(cuda)
    if mode != "flat_post":
        _param(m, key).requires_grad_(False)
    if mode != "plain":
        opt = FusedAdamW(m.parameters())
        assert all(getattr(q, "_tvq_flat", False) == q.requires_grad for q in m.parameters())
    if mode == "flat_post":
        _param(m, key).requires_grad_(False)
        _param(m, key).grad.fill_(SENTINEL)
        others = opt.flat_grad.clone()
    ref = reference(name)
    got = run(name, cuda, m=m)
    assert all(has(got["trace"], k) for k in spec.train), got["trace"]
    check_y(spec, got, ref)
    check_grads(spec, got["g"], ref["g"], skip=(key,))
    if mode == "flat_post":
        g = _param(m, key).grad
        assert torch.equal(g, torch.full_like(g, SENTINEL))
        assert g.data_ptr() >= opt.flat_grad.data_ptr() and bool((others == SENTINEL).any())
    else:
        assert _param(m, key).grad is None


@gpu
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("name", [n for n in PART2 if n != "wprod"])
def test_input_without_gradient(name, flat, cuda):
    """State 4: the inputs do not require grad (the first layer of a model): every parameter
    gradient still matches fp64, plain and flat."""
    from timevqvae.hip.optim import FusedAdamW
    spec = SPECS[name]
    m = copy.deepcopy(master(name)).to(cuda)
    if flat:
        FusedAdamW(m.parameters())
    ref = reference(name)
    got = run(name, cuda, m=m, x_grad=False)
    assert all(has(got["trace"], k) for k in spec.train), got["trace"]
    check_y(spec, got, ref)
    check_grads(spec, got["g"], ref["g"], skip=[k for k in ref["g"] if k.startswith("in")])
    assert all(v is None for k, v in got["g"].items() if k.startswith("in"))


@gpu
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("name", PART2)
def test_gradient_accumulation(name, flat, cuda):
    """State 5: two backward passes over two different inputs (and root gradients) without
    zero_grad(): the gradients are the fp64 sum of the two passes, under flat gradients
    (the kernels accumulate in place) and under plain ones (autograd accumulates)."""
    from timevqvae.hip.optim import FusedAdamW
    spec = SPECS[name]
    m = copy.deepcopy(master(name)).to(cuda)
    if flat:
        FusedAdamW(m.parameters())
    r0, r1 = reference(name, True, 0), reference(name, True, 1)
    got = run(name, cuda, m=m, seeds=(0, 1))
    assert sum(has([t], spec.train[0]) for t in got["trace"]) >= 2 if spec.train else True
    want = {k: (None if v is None else v + r1["g"][k]) for k, v in r0["g"].items()
            if not k.startswith("in")}
    check_grads(spec, got["g"], want)
    # the last pass' own output and input gradients
    check_y(spec, got, r1)
    check_grads(spec, got["g"], {k: v for k, v in r1["g"].items() if k.startswith("in")})


# ============================================================ 3. pointers and shapes
def _misaligned(m, cuda):
    """FusedAdamW over [a one-element parameter] + m's: every later pointer in the flat
    buffer is 4-byte but not 16-byte aligned."""
    from timevqvae.hip.optim import FusedAdamW
    dummy = nn.Parameter(torch.zeros(1, device=cuda))
    opt = FusedAdamW([dummy] + list(m.parameters()))
    assert all(q.data_ptr() % 16 == 4 for q in m.parameters() if q.numel() % 4 == 0)
    return opt


@gpu
@pytest.mark.parametrize("name", ["ff", "attn", "tiedce"])
def test_misaligned_parameters_fall_back(name, cuda):
    """FeedForward, the attention layer and the prior's loss head with parameters packed
    after an odd-sized one: tvq_ffn_* / tvq_attn_branch_* / tvq_tied_logits_ce reject such
    pointers, so the gates must send the layer down the per-op path (plan trace), which runs
    without raising and matches fp64, gradients in the flat buffer included."""
    spec = SPECS[name]
    m = copy.deepcopy(master(name)).to(cuda)
    opt = _misaligned(m, cuda)
    ref = reference(name)
    got = run(name, cuda, m=m)
    assert not any(has(got["trace"], k) for k in spec.train), got["trace"]
    check_y(spec, got, ref)
    check_grads(spec, got["g"], ref["g"])
    assert all(q.grad.data_ptr() >= opt.flat_grad.data_ptr() for q in m.parameters())
    # and the same unit aligned takes the fused launches
    got = run(name, cuda)
    assert all(has(got["trace"], k) for k in spec.train), got["trace"]


@gpu
def test_misaligned_lf_prior_trains(cuda):
    """The whole LF prior (embedding, one attention + feed-forward layer, head, tied CE) under
    the same misaligned flat buffer: loss and every gradient equal the aligned model's within
    1e-4 of each tensor's max-abs (the bar test_hf_embed_fold.py holds two paths of a whole
    prior to), and none of the three fused launches runs."""
    from timevqvae.hip._native import plan_trace
    from timevqvae.hip.optim import FusedAdamW
    from timevqvae.models import BidirectionalTransformer
    from timevqvae.models.bidirectional_transformer import tied_logits_ce
    torch.manual_seed(4)
    tf0 = BidirectionalTransformer("lf", 24, {"lf": 64, "hf": 64}, 128, hidden_dim=128, n_layers=1,
                                   heads=2, ff_mult=1, use_rmsnorm=True, p_unconditional=0.2,
                                   n_classes=5, model_dropout=0.0, emb_dropout=0.0)
    with torch.no_grad():
        tf0.bias.normal_(0.0, 0.1)
    g = torch.Generator().manual_seed(5)
    s = torch.randint(0, 65, (3, 24), generator=g).to(cuda)
    tgt = torch.randint(0, 64, (3, 24), generator=g).to(cuda)
    keep = (torch.rand(3, 24, generator=g) >= 0.4).to(cuda)
    one = torch.ones((), device=cuda)
    fused = ("attn_branch_fwd", "ffn_fwd", "tied_logits_ce")
    outs = []
    for mis in (False, True):
        tf = copy.deepcopy(tf0).to(cuda).train()
        _misaligned(tf, cuda) if mis else FusedAdamW(tf.parameters())
        with plan_trace() as tr:
            loss = tied_logits_ce(tf._embed_lf(s, None), tf.tok_emb_l.weight, tf.bias, 64, tgt, keep, one)
            torch.autograd.backward(loss, one)
            torch.cuda.synchronize()
        assert all(has(tr.lines, k) != mis for k in fused), tr.lines
        outs.append((loss.detach(), {k: q.grad.clone() for k, q in tf.named_parameters()}))
    (l0, g0), (l1, g1) = outs
    assert rel_max(l1, l0) < 1e-5
    for k in g0:
        if float(g0[k].abs().max()) == 0.0:  # a parameter off this loss' path
            assert float(g1[k].abs().max()) == 0.0, k
            continue
        assert rel_max(g1[k], g0[k]) < 1e-4, (k, rel_max(g1[k], g0[k]))


def _tiedce_with_bias(rows):
    torch.manual_seed(rows)
    return Holder(W=master("tiedce").W.detach().clone(), bias=_randn(rows, TCE_K + 1, scale=0.2))


BAD_ROWS = [5, 12, 48]  # neither 1 nor n = 24; 12 divides n, 48 is a multiple of it


def test_reference_bias_broadcast():
    """On the fp64 reference alone: a one-row bias broadcasts over the 24 positions, a bias
    of 5, 12 or 48 rows raises."""
    h, tgt, keep = inputs("tiedce")
    m = _tiedce_with_bias(1)
    assert torch.isfinite(ref_tiedce(Ref(m), m, h.double(), tgt, keep))
    for rows in BAD_ROWS:
        m = _tiedce_with_bias(rows)
        with pytest.raises(RuntimeError):
            ref_tiedce(Ref(m), m, h.double(), tgt, keep)


@gpu
@pytest.mark.parametrize("flat", [False, True])
def test_tied_ce_one_row_bias_broadcasts(flat, cuda):
    """A (1, K + 1) bias gives torch's broadcast result: loss, dh, dW and the (1, K + 1) bias
    gradient (summed over batch and positions) against fp64."""
    from timevqvae.hip._native import plan_trace
    from timevqvae.hip.optim import FusedAdamW
    spec = SPECS["tiedce"]
    m0 = _tiedce_with_bias(1)
    R = Ref(m0)
    h, tgt, keep = inputs("tiedce")
    hr = h.double().requires_grad_(True)
    lr = ref_tiedce(R, m0, hr, tgt, keep)
    lr.backward()
    m = copy.deepcopy(m0).to(cuda)
    if flat:
        FusedAdamW(m.parameters())
    hd = h.to(cuda).requires_grad_(True)
    with plan_trace() as tr:
        loss = fwd_tiedce(m, hd, tgt.to(cuda), keep.to(cuda))
        torch.autograd.backward(loss, m._one)
        torch.cuda.synchronize()
    assert not has(tr.lines, "tied_logits_ce"), tr.lines  # the kernel indexes rows m % rows
    assert rel_max(loss, lr) < 1e-5
    want = {"in0": hr.grad, "W": R.P["W"].grad, "bias": R.P["bias"].grad}
    check_grads(spec, {"in0": hd.grad, "W": m.W.grad, "bias": m.bias.grad}, want)


@gpu
@pytest.mark.parametrize("rows", BAD_ROWS)
def test_tied_ce_bad_bias_rows_raise(rows, cuda):
    """A bias whose row count is neither 1 nor n raises, as torch's broadcast does, from the
    fused entry point and from the unfused logits; no loss is returned."""
    from timevqvae.models.bidirectional_transformer import _TiedLogits
    m = _tiedce_with_bias(rows).to(cuda)
    h, tgt, keep = (t.to(cuda) for t in inputs("tiedce"))
    with pytest.raises((ValueError, RuntimeError)):
        fwd_tiedce(m, h.requires_grad_(True), tgt, keep)
    with pytest.raises((ValueError, RuntimeError)):
        _TiedLogits.apply(h, m.W, m.bias, TCE_K)


def _batch_slice(t):
    """t as the [::2] slice of a leaf twice as long in the batch: non-contiguous, its
    gradient the even rows of the leaf's."""
    big = torch.zeros((2 * t.shape[0],) + tuple(t.shape[1:]), device=t.device)
    big[::2] = t.detach()
    big.requires_grad_(t.requires_grad)
    v = big[::2]
    v._leaf = big
    return v


def _transposed(t):
    """t as the transpose of a leaf holding it with its last two dims swapped."""
    big = t.detach().transpose(-1, -2).contiguous().requires_grad_(t.requires_grad)
    v = big.transpose(-1, -2)
    v._leaf = big
    return v


@gpu
@pytest.mark.parametrize("view", ["slice", "transpose"])
@pytest.mark.parametrize("name", [n for n in dict.fromkeys(PART1 + PART2) if n != "wprod"])
def test_non_contiguous_inputs(name, view, cuda):
    """Every fused entry point fed a [::2] batch slice or a transposed view: the fused path
    is still taken and output, dx (through the view) and the parameter gradients match fp64;
    and the eval launch of the conv + BN blocks likewise."""
    spec = SPECS[name]
    wrap = _batch_slice if view == "slice" else _transposed
    ref = reference(name)
    got = run(name, cuda, wrap=wrap)
    assert all(not a.is_contiguous() or 1 in a.shape for a in got["args"][0]
               if a.is_floating_point())
    assert all(has(got["trace"], k) for k in spec.train), got["trace"]
    check_y(spec, got, ref)
    gin = {}
    for i, leaf in enumerate(got["leaves"][0]):
        if leaf.is_floating_point():
            gl = leaf.grad
            if view == "slice":
                assert float(gl[1::2].abs().max()) == 0.0
                gin[f"in{i}"] = gl[::2]
            else:
                gin[f"in{i}"] = gl.transpose(-1, -2)
    check_grads(spec, {**got["g"], **gin}, ref["g"])
    if name in PART1:
        ref = reference(name, False)
        got = run(name, cuda, False, False, False, wrap=wrap)
        assert all(has(got["trace"], k) for k in spec.evalm), got["trace"]
        check_y(spec, got, ref)
