"""The supervised FCN extractor's eval forward on the HIP path (tvq_fcn.hip, include/tvq_fcn.h).

Reference models/fcn.py: three ConvBlocks (Conv1dSamePadding -> BatchNorm1d -> ReLU), the mean
over positions, nn.Linear.  One `tvq_fcn_conv_bn_relu` launch per block: TensorFlow "same"
padding ((K-1)//2 on the left, the rest on the right), the eval BatchNorm folded into a
per-channel scale / shift applied in the epilogue (not into the weights, so the conv sum is the
reference's), ReLU; the third launch writes only the pooled features.  `tvq_fcn_head` is the
final Linear and, on request, the softmax.  Inference only: no autograd here; the training
step (batch statistics, the backward) is hip/fcn_train.py.
"""
import torch

from ._native import call, ptr, stream_ptr, value


def pack_weight(weight):
    """(Co, Ci, K) -> the packed form tvq_fcn_conv_bn_relu reads (tvq_fcn_pack_weight)."""
    Co, Ci, K = weight.shape
    w = weight.detach().float().contiguous()
    ptr(w)
    wp = torch.empty(max(1, value("tvq_fcn_packed_size", Co, Ci, K)), device=w.device)
    call("tvq_fcn_pack_weight", ptr(w), ptr(wp), Co, Ci, K, stream_ptr())
    return wp


def fold_bn(conv_bias, bn):
    """Eval BatchNorm1d after a biased conv as y = scale * conv + shift:
    scale = gamma / sqrt(running_var + eps), shift = beta + (bias - running_mean) * scale."""
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.float() + bn.eps)
    shift = bn.bias.detach().float() + (conv_bias.detach().float() - bn.running_mean.float()) * scale
    return scale.contiguous(), shift.contiguous()


@torch.no_grad()
def conv_bn_relu(x, weight, scale, shift, y=True, gap=False, packed=None):
    """relu(scale * conv1d_same(x, weight) + shift) for x (B, Ci, L), weight (Co, Ci, K).
    Returns (y (B, Co, L) or None, gap (B, Co) = y.mean(-1) or None); `packed` is
    pack_weight(weight) when the caller keeps it."""
    B, Ci, L = x.shape
    Co, _, K = weight.shape
    ptr(x)
    x = x.float().contiguous()
    wp = pack_weight(weight) if packed is None else packed
    out_y = torch.empty((B, Co, L), device=x.device) if y else None
    out_g = torch.empty((B, Co), device=x.device) if gap else None
    call("tvq_fcn_conv_bn_relu", ptr(x), ptr(wp), ptr(scale), ptr(shift), ptr(out_y), ptr(out_g),
         B, Ci, L, Co, K, stream_ptr())
    return out_y, out_g


@torch.no_grad()
def head(feat, weight, bias, probs=False):
    """feat (B, D) @ weight (classes, D)^T + bias -> logits (B, classes); with `probs` also the
    max-subtracted softmax: (logits, probs)."""
    B, D = feat.shape
    C = weight.shape[0]
    ptr(feat)
    feat = feat.float().contiguous()
    w = weight.detach().float().contiguous()
    b = bias.detach().float().contiguous() if bias is not None else None
    logits = torch.empty((B, C), device=feat.device)
    p = torch.empty((B, C), device=feat.device) if probs else None
    call("tvq_fcn_head", ptr(feat), ptr(w), ptr(b), ptr(logits), ptr(p), B, D, C, stream_ptr())
    return (logits, p) if probs else logits


def _key(*tensors):
    return tuple((t.data_ptr(), t._version, t.device) for t in tensors)


def _layer(module, i):
    """(weight, packed weight, scale, shift) of ConvBlock i, refolded / repacked only when a
    tensor it reads has changed (parameters and BatchNorm buffers: in-place updates move
    `_version`, a reassignment moves `data_ptr`)."""
    conv, bn = module.layers[i].layers[0], module.layers[i].layers[1]
    key = _key(conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    cache = module.__dict__.setdefault("_fcn_fold", {})
    hit = cache.get(i)
    if hit is None or hit[0] != key:
        scale, shift = fold_bn(conv.bias, bn)
        hit = cache[i] = (key, pack_weight(conv.weight), scale, shift)
    return (conv.weight,) + hit[1:]


@torch.no_grad()
def fcn_forward(module, x, return_feature_vector=False, return_probs=False):
    """FCNBaseline.forward in eval mode for x (B, C, L): the (B, 128) pooled features when
    `return_feature_vector`, else the logits, or (logits, softmax) with `return_probs`."""
    if module.training:
        raise NotImplementedError(
            "FCNBaseline training is not on the HIP path through forward(): the training step "
            "is FCNBaseline.loss(x, y) (hip.fcn_train.fcn_loss, trainers.ExpFCN); call .eval() "
            "for the features and logits")
    ptr(x)  # a CPU input is refused before anything runs
    h = x.float().contiguous()
    n = len(module.layers)
    feat = None
    for i in range(n):
        w, wp, scale, shift = _layer(module, i)
        last = i == n - 1
        h, feat = conv_bn_relu(h, w, scale, shift, y=not last, gap=last, packed=wp)
    if return_feature_vector:
        return feat
    return head(feat, module.final.weight, module.final.bias, probs=return_probs)
