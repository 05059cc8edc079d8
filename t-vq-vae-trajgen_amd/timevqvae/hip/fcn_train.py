"""The supervised FCN's training step on the HIP path (tvq_fcn_train.hip, include/tvq_fcn.h).

Reference models/fcn.py in training mode under torch.nn.CrossEntropyLoss
(scripts/train_fcn.py:101-168).  Per ConvBlock, n = B L and padL = (K-1)//2:

    u = conv1d_same(h, w) + b                      tvq_fcn_conv_train_fwd (+ fp64 partial sums)
    mean, var = biased statistics of u over (b,l)  tvq_fcn_bn_finish (+ running statistics)
    y = relu(gamma (u - mean) / sqrt(var + eps) + beta)          tvq_fcn_bn_relu

then feat = mean_l y (the third tvq_fcn_bn_relu writes only it), logits, the mean cross-entropy,
dlogits and dfeat (tvq_fcn_head_ce).  Backward: tvq_fcn_head_wgrad, and per layer from the
last tvq_fcn_bn_relu_bwd (du, dgamma, dbeta), tvq_fcn_conv_wgrad (dw, db) and
tvq_fcn_conv_dgrad (dh; layer 1 has none).

`fcn_loss(module, x, target)` is the whole network as one autograd Function, differentiable
with respect to the module's parameters (not x).  The thin wrappers above it are what the
tests pin op by op.
"""
import torch

from ._native import call, grad_buffers, ptr, stream_ptr, value
from .fcn import pack_weight


def _f(t):
    return t.detach().float().contiguous()


@torch.no_grad()
def conv_train_fwd(x, weight, bias, packed=None):
    """u = conv1d_same(x, weight) + bias (B, Co, L) and the statistics partials (2, Co, P)
    float64, P = B ceil(L / 128): sums of u and u^2 per position tile."""
    B, Ci, L = x.shape
    Co, _, K = weight.shape
    ptr(x)
    x = x.float().contiguous()
    wp = pack_weight(weight) if packed is None else packed
    b = _f(bias)
    u = torch.empty((B, Co, L), device=x.device)
    n = value("tvq_fcn_stats_size", B, L, Co)
    part = torch.empty((2, Co, n // (2 * Co)), device=x.device, dtype=torch.float64)
    call("tvq_fcn_conv_train_fwd", ptr(x), ptr(wp), ptr(b), ptr(u), ptr(part), B, Ci, L, Co, K,
         stream_ptr())
    return u, part


@torch.no_grad()
def bn_finish(part, n, gamma, beta, eps=1e-5, momentum=0.1, running_mean=None,
              running_var=None, num_batches_tracked=None):
    """stats (4, C) = mean, rstd, scale = gamma rstd, shift = beta - mean scale from the
    partials of conv_train_fwd; the running statistics are updated in place when given.
    n = B L values per channel; n = 1 raises ValueError as torch does."""
    if n < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got n = {n}")
    C, P = part.shape[1], part.shape[2]
    g, b = _f(gamma), _f(beta)
    stats = torch.empty((4, C), device=part.device)
    call("tvq_fcn_bn_finish", ptr(part), P, n, ptr(g), ptr(b), float(eps), float(momentum),
         ptr(running_mean), ptr(running_var), ptr(num_batches_tracked), ptr(stats), C,
         stream_ptr())
    return stats


@torch.no_grad()
def bn_relu(u, stats, y=True, gap=False):
    """relu(scale u + shift) (B, C, L) and / or its mean over positions (B, C)."""
    B, C, L = u.shape
    out_y = torch.empty_like(u) if y else None
    out_g = torch.empty((B, C), device=u.device) if gap else None
    call("tvq_fcn_bn_relu", ptr(u), ptr(stats), ptr(out_y), ptr(out_g), B, C, L, stream_ptr())
    return out_y, out_g


@torch.no_grad()
def head_ce(feat, weight, bias, target):
    """(logits (B, classes), loss (0-dim, the mean cross-entropy), dlogits = (softmax -
    onehot) / B, dfeat = dlogits weight (B, D)); target int64 (B,)."""
    B, D = feat.shape
    C = weight.shape[0]
    ptr(feat)
    w, b = _f(weight), _f(bias) if bias is not None else None
    t = target.reshape(-1).to(torch.int64).contiguous()
    if t.numel() != B:
        raise ValueError(f"target has {t.numel()} entries for a batch of {B}")
    dev = feat.device
    logits, dlogits = torch.empty((B, C), device=dev), torch.empty((B, C), device=dev)
    dfeat, loss = torch.empty((B, D), device=dev), torch.empty((), device=dev)
    ws = torch.empty(value("tvq_fcn_head_ce_workspace", B), device=dev)
    call("tvq_fcn_head_ce", ptr(feat), ptr(w), ptr(b), ptr(t), ptr(logits), ptr(loss),
         ptr(dlogits), ptr(dfeat), ptr(ws), B, D, C, stream_ptr())
    return logits, loss, dlogits, dfeat


@torch.no_grad()
def head_wgrad(dlogits, feat, dw=None, db=None, accumulate=False):
    """dw (+)= dlogits^T feat, db (+)= sum_b dlogits into the given buffers (None: skipped)."""
    B, C = dlogits.shape
    call("tvq_fcn_head_wgrad", ptr(dlogits), ptr(feat), ptr(dw), ptr(db), int(accumulate), B,
         feat.shape[1], C, stream_ptr())
    return dw, db


@torch.no_grad()
def bn_relu_bwd(u, stats, dy=None, dfeat=None, dgamma=None, dbeta=None, accumulate=False):
    """du of relu(BatchNorm_train(u)) from dy (B, C, L), or from dfeat (B, C) standing for
    dy = dfeat / L broadcast over l; dgamma / dbeta (+)= into the given buffers (None:
    skipped)."""
    B, C, L = u.shape
    du = torch.empty_like(u)
    ws = torch.empty(value("tvq_fcn_bn_bwd_workspace", B, C), device=u.device, dtype=torch.float64)
    call("tvq_fcn_bn_relu_bwd", ptr(u), ptr(dy), ptr(dfeat), ptr(stats), ptr(du), ptr(dgamma),
         ptr(dbeta), int(accumulate), ptr(ws), B, C, L, stream_ptr())
    return du


@torch.no_grad()
def pack_weight_t(weight):
    """(Co, Ci, K) -> the data gradient's operand: the flipped transpose, packed."""
    Co, Ci, K = weight.shape
    w = _f(weight)
    ptr(w)
    wpt = torch.empty(max(1, value("tvq_fcn_packed_size", Ci, Co, K)), device=w.device)
    call("tvq_fcn_pack_weight_t", ptr(w), ptr(wpt), Co, Ci, K, stream_ptr())
    return wpt


@torch.no_grad()
def conv_dgrad(du, weight, packed_t=None):
    """dh (B, Ci, L) of u = conv1d_same(h, weight) from du (B, Co, L)."""
    B, Co, L = du.shape
    _, Ci, K = weight.shape
    wpt = pack_weight_t(weight) if packed_t is None else packed_t
    dh = torch.empty((B, Ci, L), device=du.device)
    call("tvq_fcn_conv_dgrad", ptr(du), ptr(wpt), ptr(dh), B, Ci, L, Co, K, stream_ptr())
    return dh


@torch.no_grad()
def conv_wgrad(du, h, K, dw=None, db=None, accumulate=False):
    """dw (Co, Ci, K) (+)= sum_{b,l} du h shifted, db (Co) (+)= sum_{b,l} du into the given
    buffers (None: skipped; not both)."""
    B, Co, L = du.shape
    Ci = h.shape[1]
    ws = torch.empty(max(1, value("tvq_fcn_conv_wgrad_workspace", B, Ci, L, Co, K)), device=du.device)
    call("tvq_fcn_conv_wgrad", ptr(du), ptr(h), ptr(dw), ptr(db), int(accumulate), ptr(ws), B, Ci,
         L, Co, K, stream_ptr())
    return dw, db


def _blocks(module):
    return [(blk.layers[0], blk.layers[1]) for blk in module.layers]


class _FCNLoss(torch.autograd.Function):
    """inputs: x, target, then per ConvBlock (conv.weight, conv.bias, bn.weight, bn.bias) and
    final.weight, final.bias.  Saves u_i, stats_i and the ConvBlocks' inputs."""

    @staticmethod
    def forward(ctx, module, x, target, *params):
        blocks = _blocks(module)
        n = x.shape[0] * x.shape[2]
        h, saved, feat = x, [], None
        for i, (conv, bn) in enumerate(blocks):
            w, b, g, be = params[4 * i:4 * i + 4]
            u, part = conv_train_fwd(h, w, b)
            stats = bn_finish(part, n, g, be, bn.eps, bn.momentum, bn.running_mean,
                              bn.running_var, bn.num_batches_tracked)
            last = i == len(blocks) - 1
            y, gap = bn_relu(u, stats, y=not last, gap=last)
            saved += [h, u, stats]
            h, feat = y, gap
        fw, fb = params[-2], params[-1]
        logits, loss, dlogits, dfeat = head_ce(feat, fw, fb, target)
        ctx.params = params
        ctx.nblocks = len(blocks)
        ctx.save_for_backward(feat, dlogits, dfeat, *saved, *[_f(p) for p in params[:-2:4]])
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    @torch.no_grad()
    def backward(ctx, gloss, _glogits):
        t = ctx.saved_tensors
        nb, params = ctx.nblocks, ctx.params
        feat, dlogits, dfeat = t[:3]
        saved, weights = t[3:3 + 3 * nb], t[3 + 3 * nb:]
        need = ctx.needs_input_grad[3:]
        out = [None] * len(params)

        def buffers(idx):
            """grad buffers of params[idx] that need one (else None), and whether they are the
            optimizer's sinks: the kernels then accumulate and autograd gets None"""
            ps = [params[k] if need[k] else None for k in idx]
            if all(p is None for p in ps):
                return [None] * len(idx), True
            return grad_buffers(ps)

        def give(idx, bufs, direct):
            if not direct:
                for k, b in zip(idx, bufs):
                    out[k] = b

        dlogits, dfeat = dlogits * gloss, dfeat * gloss
        idx = (len(params) - 2, len(params) - 1)
        bufs, direct = buffers(idx)
        if any(b is not None for b in bufs):
            head_wgrad(dlogits, feat, bufs[0], bufs[1], direct)
        give(idx, bufs, direct)

        dy = None
        for i in reversed(range(nb)):
            h, u, stats = saved[3 * i:3 * i + 3]
            K = weights[i].shape[2]
            idx = (4 * i + 2, 4 * i + 3)
            bufs, direct = buffers(idx)
            du = bn_relu_bwd(u, stats, dy=dy, dfeat=dfeat if dy is None else None,
                             dgamma=bufs[0], dbeta=bufs[1], accumulate=direct)
            give(idx, bufs, direct)
            idx = (4 * i, 4 * i + 1)
            bufs, direct = buffers(idx)
            if any(b is not None for b in bufs):  # a frozen conv runs no weight gradient
                conv_wgrad(du, h, K, bufs[0], bufs[1], direct)
            give(idx, bufs, direct)
            if i > 0:
                dy = conv_dgrad(du, weights[i])
        return (None, None, None) + tuple(out)


def fcn_loss(module, x, target):
    """(loss, logits) of FCNBaseline `module` in training mode for x (B, C, L) and the int64
    class indices `target` (B,) or (B, 1): the reference's `criterion(fcn(x), y)`.  `loss` (a
    0-dim device tensor) carries the gradient of every parameter with requires_grad; a frozen
    parameter gets none and its launch is skipped where one exists.  The BatchNorm running
    statistics and num_batches_tracked are updated as torch updates them."""
    if not module.training:
        raise RuntimeError("fcn_loss needs the module in training mode (module.train()); "
                           "the eval forward is FCNBaseline.forward")
    ptr(x)  # a CPU input is refused before anything runs
    B, _, L = x.shape
    if B * L < 2:
        raise ValueError("Expected more than 1 value per channel when training, got input size "
                         f"{tuple(x.shape)}")
    for _, bn in _blocks(module):
        if bn.momentum is None or not bn.track_running_stats:
            raise NotImplementedError("FCN training needs BatchNorm1d with a momentum and "
                                      "running statistics")
    module.__dict__.pop("_fcn_fold", None)  # the eval path's fold of the old statistics
    params = []
    for conv, bn in _blocks(module):
        params += [conv.weight, conv.bias, bn.weight, bn.bias]
    params += [module.final.weight, module.final.bias]
    target = target.reshape(-1).to(device=x.device, dtype=torch.int64)
    return _FCNLoss.apply(module, x.detach().float().contiguous(), target, *params)
