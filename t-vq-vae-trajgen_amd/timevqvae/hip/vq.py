"""VQ codebook ops on the HIP path (include/tvq.h §VQ codebook).

Replaces EuclideanCodebook.forward + the straight-through/commitment part of
VectorQuantize.forward (reference timevqvae/models/vq.py:197-251, 357-366):
  assign (L2 + argmin + gather, fp32 MFMA)  ->  per-code stats (deterministic)
  -> [optional all-reduce of the stats: sync_codebook, vq.py:229,234]
  -> EMA blend -> Laplace-normalised codebook + perplexity + commit loss
  -> [threshold_ema_dead_code > 0: dead codes re-seeded from the batch, vq.py:187-195, 243].
The k-means codebook initialisation (kmeans_init, vq.py:67-106, 170-179) is `kmeans_init`:
a one-off fit, enqueued whole with no host synchronisation.
"""
import contextlib

import torch

from . import rng, streams
from ._native import call, ptr, stream_ptr, value

_SVQ_SITE = 0x5F << 56  # noise stream of the stochastic assignment (svq_temp > 0); fixed, so
# module-construction site numbering (rng.new_site) is unchanged
_KMEANS_SITE = 0x5E << 56  # row draw of the k-means initialisation (kmeans_init)
_EXPIRE_SITE = 0x5D << 56  # row draw of the dead-code expiry (threshold_ema_dead_code > 0)

_pending = None  # list of CodebookUpdate while a deferral scope is active


class CodebookUpdate:
    """An EMA codebook update whose per-batch statistics are computed but not yet applied.

    The forward outputs never read the updated codebook (quantize = E_old[idx]), so the
    update can move after the backward: `reduce()` runs the sync_codebook all-reduce of
    the statistics (eager, between captured graph segments) and `apply()` the EMA blend +
    Laplace-normalised codebook (capturable).

    threshold > 0: the dead-code expiry (vq.py:243 expire_codes_) follows the renormalised
    codebook in `apply()`: codes whose post-EMA cluster_size is below the threshold are
    re-seeded from `rows` (the pass's token rows, (B,N,D), any dense strides), at the rows
    `sel` (int32 (K,), tests) or at rows the kernel draws from the device seed at `offset`.
    """

    def __init__(self, cs_b, es_b, cluster_size, embed_avg, embed, decay, eps, sync, *,
                 rows=None, threshold=0, sel=None, offset=0):
        self.cs_b, self.es_b = cs_b, es_b
        self.cluster_size, self.embed_avg, self.embed = cluster_size, embed_avg, embed
        self.decay, self.eps, self.sync = decay, eps, sync
        self.K, self.D = embed.shape
        self.rows, self.threshold, self.sel, self.offset = rows, threshold, sel, offset

    def reduce(self):
        if self.sync is not None:
            self.sync(self.cs_b)
            self.sync(self.es_b)

    def apply(self):
        s = stream_ptr()
        call("tvq_vq_ema", ptr(self.cs_b), ptr(self.es_b), self.K, self.D, float(self.decay),
             ptr(self.cluster_size), ptr(self.embed_avg), s)
        call("tvq_vq_finalize", ptr(self.cluster_size), ptr(self.embed_avg), self.K, self.D,
             float(self.eps), ptr(self.embed), None, 0, None, None, 0, None, s)
        if self.threshold > 0:
            expire(self.rows, self.embed, self.cluster_size, self.threshold, sel=self.sel,
                   offset=self.offset)


@contextlib.contextmanager
def deferred_codebook_updates():
    """Collect the EMA codebook updates of the passes run inside the scope instead of
    applying them; yields the list of CodebookUpdate (reduce() then apply() each)."""
    global _pending
    prev, _pending = _pending, []
    try:
        yield _pending
    finally:
        _pending = prev


_indices_only = [False]


@contextlib.contextmanager
def indices_only():
    """Eval codebook passes in the body skip the per-code counts and the perplexity (their
    group-by and reductions): for callers that read only the indices, such as MaskGIT's
    frozen tokenizer (maskgit.py:117-134 discards the perplexity).  Training passes are
    unaffected (their EMA needs the statistics)."""
    prev = _indices_only[0]
    _indices_only[0] = True
    try:
        yield
    finally:
        _indices_only[0] = prev


def _same_dense_layout(a, b):
    return a.shape == b.shape and a.stride() == b.stride()


def _check_dense(x):
    order = sorted(range(x.dim()), key=lambda i: -x.stride(i))
    if not x.permute(order).is_contiguous():
        raise ValueError("tvq VQ: input must be a dense (possibly permuted) tensor")


def _rows3(x):
    """x as (B,N,D): a (M,D) matrix becomes (1,M,D), other ranks are flattened token-major."""
    if x.dim() == 3:
        return x
    return x.unsqueeze(0) if x.dim() == 2 else x.reshape(1, -1, x.shape[-1])


def draw_rows(M, K, device, offset=None, site=_KMEANS_SITE):
    """sample_vectors' row choice (vq.py:67-75) drawn on the device: int32 (K,) row indices
    in [0, M), distinct when M >= K, i.i.d. uniform otherwise.  Keyed on the device seed
    (hip/rng.py) and `offset` (None: the next call offset of `site`)."""
    sel = torch.empty(K, device=device, dtype=torch.int32)
    off = rng.call_offset(site) if offset is None else int(offset) & 0xFFFFFFFFFFFFFFFF
    call("tvq_vq_draw_rows", M, K, ptr(rng.seed_tensor(device)), off, ptr(sel), stream_ptr())
    return sel


def _check_sel(sel, K):
    if sel.shape != (K,) or sel.dtype != torch.int32 or not sel.is_contiguous():
        raise ValueError("vq: injected row indices must be a contiguous int32 (K,) tensor")


def kmeans_init(x, K, iters, sel=None):
    """kmeans (vq.py:78-106) of the token rows x ((B,N,D) or (M,D), dense, any strides) into
    K clusters, `iters` Lloyd iterations, starting from the rows `sel` (int32 (K,); None:
    drawn on the device, draw_rows).  Returns (means (K,D), bins (K,) float).  Enqueued
    whole on the current stream, no host synchronisation; deterministic."""
    x = _rows3(x)
    B, N, D = x.shape
    M = B * N
    _check_dense(x)
    dev = x.device
    if sel is None:
        sel = draw_rows(M, K, dev)
    _check_sel(sel, K)
    means = torch.empty((K, D), device=dev, dtype=torch.float32)
    bins = torch.empty(K, device=dev, dtype=torch.float32)
    ws = torch.empty(value("tvq_vq_kmeans_workspace", M, K, D), device=dev, dtype=torch.int32)
    sB, sN, sD = x.stride()
    call("tvq_vq_kmeans", ptr(x), B, N, D, sB, sN, sD, ptr(sel), K, int(iters), ptr(means),
         ptr(bins), ptr(ws), stream_ptr())
    return means, bins


def expire(x, embed, cluster_size, threshold, sel=None, offset=None, n_expired=None):
    """expire_codes_ (vq.py:187-195) in one capturable launch: embed[k] = x row sel[k] for
    every k with cluster_size[k] < threshold; nothing else is written.  sel None: the kernel
    draws the rows from the device seed at `offset` (None: the next call offset of the
    expiry site).  n_expired: optional int32 (1,) tensor that receives the expired count."""
    x = _rows3(x)
    B, N, D = x.shape
    K = embed.shape[0]
    _check_dense(x)
    if embed.shape[1] != D:
        raise ValueError("vq: expiry rows and codebook differ in dim")
    seed = None
    off = 0
    if sel is None:
        seed = rng.seed_tensor(x.device)
        off = rng.call_offset(_EXPIRE_SITE) if offset is None else int(offset)
    else:
        _check_sel(sel, K)
    sB, sN, sD = x.stride()
    call("tvq_vq_expire", ptr(x), B, N, D, sB, sN, sD, ptr(sel), ptr(seed), off,
         ptr(cluster_size), float(threshold), K, ptr(embed), ptr(n_expired), stream_ptr())


def vq_codebook_pass(x, embed, cluster_size, embed_avg, *, straight_through, ema, decay, eps,
                     sync=None, svq_temp=None, gumbel=None, expire_threshold=0,
                     expire_sel=None):
    """One codebook pass over x (B,N,D).

    svq_temp > 0: stochastic assignment idx ~ Categorical(softmax(dist / svq_temp))
    (vq.py:51-56, 216-222), drawn on the device by Gumbel-max; `gumbel` (M, K) injects the
    noise (tests), otherwise it comes from the device seed (hip/rng.py).

    Returns (out, idx, commit, perplexity, counts):
      out   = x + (E[idx]-x) if straight_through else E[idx]  (pre-update codebook)
      idx   = int64 (B,N);  commit = mean((out-x)^2) (0-dim) if straight_through else None
      perplexity 0-dim;     counts = int32 (K,)
    With ema=True the buffers cluster_size/embed_avg/embed are updated in place, and
    expire_threshold > 0 then re-seeds the dead codes from x's rows (vq.py:243; `expire_sel`
    injects the row choice, tests).
    """
    B, N, D = x.shape
    K = embed.shape[0]
    M = B * N
    _check_dense(x)
    dev = x.device
    streams.wait_fence(embed.data_ptr())  # an EMA update of this codebook may be in flight
    s = stream_ptr()
    ee = torch.empty(K, device=dev, dtype=torch.float32)
    call("tvq_vq_sqnorm", ptr(embed), K, D, ptr(ee), s)
    out = torch.empty_like(x)
    assert _same_dense_layout(out, x)
    idx = torch.empty((B, N), device=dev, dtype=torch.long)
    idx32 = torch.empty(M, device=dev, dtype=torch.int32)
    nb = value("tvq_vq_assign_nblocks", M)
    partial = torch.empty(nb, device=dev, dtype=torch.float32) if straight_through else None
    sB, sN, sD = x.stride()
    # EMA statistics sum token rows per code: with an NCHW latent (sD > 1) the assign pass
    # also writes x token-major so that those sums read contiguous rows
    rows = (torch.empty((M, D), device=dev, dtype=torch.float32)
            if ema and straight_through and sD != 1 else None)
    if svq_temp and gumbel is not None and (gumbel.shape != (M, K) or not gumbel.is_contiguous()):
        raise ValueError("vq: injected gumbel noise must be a contiguous (M, K) tensor")
    seed, off = rng.draw(dev, _SVQ_SITE, bool(svq_temp) and gumbel is None)
    call("tvq_vq_assign_rows", ptr(x), B, N, D, sB, sN, sD, ptr(embed), ptr(ee), K,
         int(bool(straight_through)), float(svq_temp or 0.0), ptr(gumbel), ptr(seed), off,
         ptr(out), ptr(idx), ptr(idx32), ptr(partial), ptr(rows), s)
    commit = torch.empty((), device=dev, dtype=torch.float32) if straight_through else None
    # the commitment mean is read only by the loss report at the band's end (its gradient
    # does not need it): it joins the statistics' finish launch unless those are skipped or
    # offloaded to another stream (then it is finished here, on the current stream)
    late = not (_indices_only[0] and not ema) and "vq" not in streams.OFFLOAD
    if straight_through and not late:
        call("tvq_vq_finalize", None, None, K, D, float(eps), None, None, M, None, ptr(partial),
             nb, ptr(commit), s)
    # per-code statistics, EMA and perplexity: nothing downstream of the quantised output
    # waits for them (inside streams.concurrent() they run on the aux stream; the region's
    # join completes them before anyone reads the perplexity or the codebook)
    if _indices_only[0] and not ema:
        return out, idx, commit, None, None
    src = rows.view(1, M, D) if rows is not None else x
    cm = (partial, nb, commit) if straight_through and late else (None, 0, None)
    with streams.offload(src, idx32, kind="vq"):
        counts, perp = _codebook_stats(src, idx32, embed, cluster_size, embed_avg, ema, decay,
                                       eps, sync, cm, expire_threshold, expire_sel)
    return out, idx, commit, perp, counts


def _codebook_stats(x, idx32, embed, cluster_size, embed_avg, ema, decay, eps, sync,
                    cm=(None, 0, None), expire_threshold=0, expire_sel=None):
    """cm = (commit partials, their count, commit): the commitment mean, finished by the
    same vq_finalize launch as the perplexity.  expire_threshold > 0 (with ema): the
    dead-code expiry from the rows of x follows the renormalised codebook."""
    cpart, nb, commit = cm
    B, N, D = x.shape
    K = embed.shape[0]
    M = B * N
    dev = x.device
    sB, sN, sD = x.stride()
    s = stream_ptr()
    counts = torch.empty(K, device=dev, dtype=torch.int32)
    cs_b = torch.empty(K, device=dev, dtype=torch.float32)
    es_b = torch.empty((K, D), device=dev, dtype=torch.float32) if ema else None
    ws = torch.empty(value("tvq_vq_stats_workspace", M, K), device=dev, dtype=torch.int32)
    call("tvq_vq_stats", ptr(x), B, N, D, sB, sN, sD, ptr(idx32), K, ptr(counts), ptr(cs_b),
         ptr(es_b), ptr(ws), s)
    perp = torch.empty((), device=dev, dtype=torch.float32)
    xoff = 0
    if ema and expire_threshold > 0 and expire_sel is None:
        xoff = rng.call_offset(_EXPIRE_SITE)  # drawn here, so a deferred apply() uses the same
    if ema and _pending is not None:
        if expire_threshold > 0:
            upd = CodebookUpdate(cs_b, es_b, cluster_size, embed_avg, embed, decay, eps, sync,
                                 rows=x, threshold=expire_threshold, sel=expire_sel, offset=xoff)
        else:
            upd = CodebookUpdate(cs_b, es_b, cluster_size, embed_avg, embed, decay, eps, sync)
        _pending.append(upd)
        call("tvq_vq_finalize", None, None, K, D, float(eps), None, ptr(counts), M, ptr(perp),
             ptr(cpart), nb, ptr(commit), s)
    elif ema:
        if sync is not None:
            sync(cs_b)
            sync(es_b)
            s = stream_ptr()
        call("tvq_vq_ema", ptr(cs_b), ptr(es_b), K, D, float(decay), ptr(cluster_size),
             ptr(embed_avg), s)
        call("tvq_vq_finalize", ptr(cluster_size), ptr(embed_avg), K, D, float(eps), ptr(embed),
             ptr(counts), M, ptr(perp), ptr(cpart), nb, ptr(commit), s)
        if expire_threshold > 0:
            expire(x, embed, cluster_size, expire_threshold, sel=expire_sel, offset=xoff)
        streams.fence(embed.data_ptr())
    else:
        call("tvq_vq_finalize", None, None, K, D, float(eps), None, ptr(counts), M, ptr(perp),
             ptr(cpart), nb, ptr(commit), s)
    return counts, perp


class _VQStraightThrough(torch.autograd.Function):
    """Training pass: forward = codebook pass with EMA; backward of vq.py:358,364."""

    @staticmethod
    def forward(ctx, x, embed, cluster_size, embed_avg, ema, decay, eps, sync, svq_temp,
                expire_threshold=0, expire_sel=None):
        out, idx, commit, perp, _ = vq_codebook_pass(
            x, embed, cluster_size, embed_avg, straight_through=True, ema=ema, decay=decay,
            eps=eps, sync=sync, svq_temp=svq_temp, expire_threshold=expire_threshold,
            expire_sel=expire_sel)
        ctx.save_for_backward(x, out)
        ctx.mark_non_differentiable(idx, perp)
        ctx.set_materialize_grads(False)  # no zero-filled grads for idx / perp (None handled)
        return out, idx, commit, perp

    @staticmethod
    def backward(ctx, g_out, g_idx, g_commit, g_perp):
        x, out = ctx.saved_tensors
        if g_out is None:
            g_out = torch.zeros_like(x)
        elif not _same_dense_layout(g_out, x):
            g = torch.empty_like(x)
            g.copy_(g_out)
            g_out = g
        dx = torch.empty_like(x)
        gc = g_commit.contiguous() if g_commit is not None else None
        call("tvq_vq_backward", ptr(x), ptr(out), ptr(g_out), ptr(gc), x.numel(), x.numel(),
             ptr(dx), stream_ptr())
        return (dx,) + (None,) * 10


def vq_train(x, embed, cluster_size, embed_avg, *, ema, decay, eps, sync=None, svq_temp=None,
             expire_threshold=0, expire_sel=None):
    """Training-mode VQ with straight-through gradient. Returns (out, idx, commit, perp)."""
    return _VQStraightThrough.apply(x, embed, cluster_size, embed_avg, ema, decay, eps, sync,
                                    svq_temp, expire_threshold, expire_sel)
