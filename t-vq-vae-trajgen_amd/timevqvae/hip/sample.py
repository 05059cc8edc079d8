"""MaskGIT sampling ops on the HIP path (include/tvq.h §MaskGIT sampling).

maskgit_sample + maskgit_remask together are one step of first_pass / second_pass
(reference maskgit.py:294-411); codebook_gather_nchw is the codebook lookup of
decode_token_ind_to_timeseries (maskgit.py:461-469)."""
import numpy as np
import torch

from . import rng
from ._native import call, ptr, stream_ptr, value


def mask_len(unknown0: int, mask_ratio: float) -> int:
    """floor(unknown0 * mask_ratio) in float32, clipped at 0 (maskgit.py:328-333)."""
    return max(0, int(np.floor(np.float32(unknown0) * np.float32(mask_ratio))))


def full_tokens(shape, value, device):
    """torch.full(shape, value, int64) on the HIP path (tvq_fill_i64): the all-masked token
    rows of MaskGIT.create_input_tokens_normal (maskgit.py:230-236)."""
    t = torch.empty(shape, dtype=torch.int64, device=device)
    if t.is_cuda:
        call("tvq_fill_i64", ptr(t), t.numel(), int(value), stream_ptr())
    else:
        t.fill_(int(value))
    return t


def maskgit_sample(logits, s, mask_id, gumbel=None, site=0):
    """(sampled ids with known tokens kept, p(sampled) with +inf for known tokens).

    The draw is Categorical(logits).sample() as torch runs it -- torch.multinomial's
    n_sample = 1 exponential race, argmax_k l_k + Gumbel_k (maskgit.py:307-315) -- with the
    Gumbel noise from the device seed's counter hash, or `gumbel` (B, n, K) when given."""
    B, n, K = logits.shape
    sb, sn, sk = logits.stride()
    if sk != 1:
        raise ValueError("maskgit_sample: logits must be contiguous along the code axis")
    s = s.contiguous()
    sampled = torch.empty_like(s)
    selp = torch.empty((B, n), device=logits.device, dtype=torch.float32)
    seed, off = rng.draw(logits.device, site, gumbel is None)
    call("tvq_maskgit_sample", ptr(logits), sb, sn, B, n, K, ptr(s), int(mask_id),
         ptr(gumbel.contiguous() if gumbel is not None else None), ptr(seed), off, ptr(sampled),
         ptr(selp), stream_ptr())
    return sampled, selp


_tls_ws = {}


def _tls_workspace(dev, K, D, nb):
    key = (dev, K, D, nb)
    ws = _tls_ws.get(key)
    if ws is None:
        nbytes = value("tvq_tied_logits_sample_workspace", K, D, nb)
        if nbytes < 0:
            raise ValueError("tied_logits_sample: unsupported shape")
        ws = torch.empty((nbytes + 15) // 16 * 4, device=dev, dtype=torch.float32)
        _tls_ws[key] = ws
    return ws


def _tied_logits_sample(h, h_null, cfg_scale, W, bias, K, s, mask_id, gumbel, site, want_logits):
    """Both draws below.  h_null None: tvq_tied_logits_sample on h; else the guided entry on
    (h, h_null) with cfg_scale."""
    B, n, D = h.shape
    M = B * n
    hs = [t.reshape(M, D).contiguous() for t in ((h,) if h_null is None else (h, h_null))]
    s = s.contiguous()
    dev = h.device
    nb = bias.shape[0]
    ws = _tls_workspace(dev, K, D, nb)
    sampled = torch.empty_like(s)
    selp = torch.empty((B, n), device=dev, dtype=torch.float32)
    logits = torch.empty((B, n, K), device=dev, dtype=torch.float32) if want_logits else None
    seed, off = rng.draw(dev, site, gumbel is None)
    shape = (M, D, ptr(W.contiguous()), K, ptr(bias), nb, bias.stride(0))
    guide = () if h_null is None else (float(cfg_scale),)
    call("tvq_tied_logits_sample" if h_null is None else "tvq_tied_logits_sample_cfg",
         *[ptr(t) for t in hs], *shape, *guide, ptr(s), int(mask_id),
         ptr(gumbel.contiguous() if gumbel is not None else None), ptr(seed), off,
         ptr(sampled), ptr(selp), ptr(logits), ptr(ws), stream_ptr())
    return (sampled, selp, logits) if want_logits else (sampled, selp)


def tied_logits_sample(h, W, bias, K, s, mask_id, gumbel=None, site=0, want_logits=False):
    """maskgit_sample(h @ W[:K]^T + bias[:, :K], s, mask_id) in one pass: the tied logits of
    the prior's head (bidirectional_transformer.py:186-191) computed on MFMA and consumed by
    the race in registers, never written to memory (include/tvq.h tvq_tied_logits_sample).
    h (B, n, D) with D 64 or 128; bias (n, ldb >= K).  want_logits: also return the logits
    the draw used (tests)."""
    return _tied_logits_sample(h, None, None, W, bias, K, s, mask_id, gumbel, site, want_logits)


def tied_logits_sample_cfg(h_cond, h_null, W, bias, K, s, mask_id, cfg_scale, gumbel=None,
                           site=0, want_logits=False):
    """tied_logits_sample on the classifier-free-guidance mix (maskgit.py:136-153):
    l_null + cfg_scale * (l_cond - l_null) with l_x = h_x @ W[:K]^T + bias[:, :K], the code
    table read once for both branches and neither branch's logits written
    (tvq_tied_logits_sample_cfg).  h_cond, h_null (B, n, D); the logits returned with
    want_logits are the mix."""
    if h_cond.shape != h_null.shape:
        raise ValueError("tied_logits_sample_cfg: h_cond and h_null differ in shape")
    return _tied_logits_sample(h_cond, h_null, cfg_scale, W, bias, K, s, mask_id, gumbel, site,
                               want_logits)


def maskgit_remask(selp, k, temperature, sampled=None, mask_id=0, u_gumbel=None, site=0,
                   want_masking=False):
    """Re-mask the k lowest-confidence tokens per row.  Returns s_out (if sampled given)
    and/or the bool masking (want_masking)."""
    B, n = selp.shape
    dev = selp.device
    s_out = torch.empty_like(sampled) if sampled is not None else None
    masking = torch.empty((B, n), device=dev, dtype=torch.uint8) if want_masking else None
    seed, off = rng.draw(dev, site, u_gumbel is None)
    call("tvq_maskgit_remask", ptr(selp.contiguous()), B, n, int(k), float(temperature),
         ptr(u_gumbel.contiguous() if u_gumbel is not None else None), ptr(seed), off,
         ptr(sampled), int(mask_id), ptr(s_out), ptr(masking), stream_ptr())
    if want_masking:
        return (s_out, masking.bool()) if s_out is not None else masking.bool()
    return s_out


def codebook_gather_nchw(s, E, H, W):
    """E[s] laid out (b, d, H, W) for the decoder (s: (b, H*W) int64, E: (K, d))."""
    B, P = s.shape
    K, D = E.shape
    if P != H * W:
        raise ValueError("codebook_gather_nchw: token count != H*W")
    out = torch.empty((B, D, H, W), device=E.device, dtype=torch.float32)
    call("tvq_codebook_gather_nchw", ptr(s.contiguous()), B, P, D, ptr(E.contiguous()), ptr(out),
         stream_ptr())
    return out
