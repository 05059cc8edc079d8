"""Generate the G12 goldens (k-means codebook init and dead-code expiry) from the REFERENCE
timevqvae/models/vq.py (kmeans vq.py:78-106, init_embed_ / replace / expire_codes_
vq.py:170-195, 243).

Runs only where the reference checkout exists (the build container); the reference file is
loaded by path exactly as make_golden.py does.  Only the .npz outputs are committed:

    tests/golden/g12_vq_init.npz       k-means cases 1, 2, 5 and the two expiry cases
    tests/golden/g12_vq_init_c3.npz    k-means case 3
    tests/golden/g12_vq_init_c4.npz    k-means case 4

(three files: float32 noise does not compress and a committed file stays below 1 MiB).

Before anything is written the generator asserts, at every one of the 10 iterations of every
k-means case, that the reference's fp32 buckets equal those of the same recurrence in fp64
and that no sample's best and second-best squared distances (fp64, distinct candidate means)
are closer than 1e-5 relative: the HIP path evaluates the distance in the expansion form
|x|^2 - 2 x.m + |m|^2, which may pick another bucket only at such near ties.

    python tests/golden/make_golden_vq_init.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, _load  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
DATA_SEED = 1234
ITERS = (1, 2, 10)
MIN_REL_GAP = 1e-5

# name -> (M, K, D, data kind, init seed, output file)
CASES = {
    "c1": (1000, 32, 32, "randn", 7, "g12_vq_init.npz"),
    "c2": (1000, 32, 32, "blobs", 7, "g12_vq_init.npz"),
    "c3": (2000, 96, 64, "randn", 7, "g12_vq_init_c3.npz"),
    # init seed 8: with seed 7 one sample of iteration 4 sits at a relative gap of 7e-6
    "c4": (1536, 130, 128, "randn", 8, "g12_vq_init_c4.npz"),
    "c5": (40, 64, 32, "randn", 7, "g12_vq_init.npz"),
}


def make_data(M, K, D, kind):
    torch.manual_seed(DATA_SEED)
    if kind == "randn":
        return torch.randn(M, D)
    c = 2.0 * torch.randn(K, D)
    return c[torch.randint(0, K, (M,))] + 0.3 * torch.randn(M, D)


def draw(M, K, seed):
    """sample_vectors' indices (vq.py:67-75) for the generator state `seed`."""
    torch.manual_seed(seed)
    if M >= K:
        return torch.randperm(M)[:K]
    return torch.randint(0, M, (K,))


def lloyd_step(x, means):
    """One iteration of vq.py:83-104 (Euclidean) in x's dtype; returns (means, bins, buckets, dist)."""
    K, D = means.shape
    d = ((x[:, None, :] - means[None, :, :]) ** 2).sum(-1)
    buckets = (-d).max(dim=-1).indices
    bins = torch.bincount(buckets, minlength=K)
    zero = bins == 0
    new = torch.zeros(K, D, dtype=x.dtype)
    new.scatter_add_(0, buckets[:, None].expand(-1, D), x)
    new = new / bins.masked_fill(zero, 1)[:, None]
    return torch.where(zero[:, None], means, new), bins, buckets, d


def min_rel_gap(d, means, buckets):
    """Smallest (second - best) / second squared distance over the samples, the second best
    taken among clusters whose mean differs from the best's (duplicate means tie exactly)."""
    same = (means[:, None, :] == means[None, :, :]).all(-1)  # (K, K)
    dd = d.clone()
    dd[same[buckets]] = float("inf")
    second = dd.min(-1).values
    best = d.gather(1, buckets[:, None])[:, 0]
    ok = torch.isfinite(second)
    return float(((second - best) / second)[ok].min()) if ok.any() else float("inf")


def gen_kmeans(ref, name, M, K, D, kind, seed):
    x = make_data(M, K, D, kind)
    sel = draw(M, K, seed)
    out = {f"{name}_x": x.numpy(), f"{name}_sel": sel.numpy().astype(np.int32)}
    # the conditions, iteration by iteration: fp32 (the reference's arithmetic) next to fp64
    m32, m64 = x[sel], x[sel].double()
    x64 = x.double()
    gaps = []
    for it in range(max(ITERS)):
        m32, bins32, b32, _ = lloyd_step(x, m32)
        means64_before = m64
        m64, _, b64, d64 = lloyd_step(x64, m64)
        assert torch.equal(b32, b64), f"{name} iteration {it}: fp32 / fp64 buckets differ"
        gaps.append(min_rel_gap(d64, means64_before, b64))
        assert gaps[-1] >= MIN_REL_GAP, f"{name} iteration {it}: relative gap {gaps[-1]:.3g}"
    for iters in ITERS:
        torch.manual_seed(seed)
        means, bins = ref.vq.kmeans(x, K, iters)
        # the step-wise restatement above is the reference's recurrence
        m = x[sel]
        for _ in range(iters):
            m, b, bk, _ = lloyd_step(x, m)
        assert torch.equal(m, means) and torch.equal(b, bins), f"{name}: sel does not reproduce kmeans"
        out[f"{name}_means{iters}"] = means.numpy()
        out[f"{name}_bins{iters}"] = bins.numpy().astype(np.int32)
        out[f"{name}_buckets{iters}"] = bk.numpy().astype(np.int16)
    drift = float((m32 - m64.float()).abs().max())
    print(f"{name}: M={M} K={K} D={D} {kind}: min rel gap {min(gaps):.3g}, empty clusters "
          f"{int((bins == 0).sum())}, fp32/fp64 mean drift {drift:.2g}")
    return out


def gen_expire(ref, name, shape, seed):
    K, D, thr = 64, 32, 2
    g = torch.Generator().manual_seed(DATA_SEED + len(name) + shape[0])
    x = torch.randn(*shape, generator=g)
    vqm = ref.vq.VectorQuantize(dim=D, codebook_size=K, decay=0.8, threshold_ema_dead_code=thr)
    vqm.train()
    cb = vqm._codebook
    cb.embed.data.copy_(torch.randn(K, D, generator=g))
    cb.embed_avg.data.copy_(torch.randn(K, D, generator=g))
    cb.cluster_size.data.copy_(4.0 * torch.rand(K, generator=g))
    out = {f"{name}_x": x.numpy().copy(), f"{name}_embed": cb.embed.numpy().copy(),
           f"{name}_embed_avg": cb.embed_avg.numpy().copy(),
           f"{name}_cluster_size": cb.cluster_size.numpy().copy()}
    torch.manual_seed(seed)
    _, ind, _, _ = vqm(x)
    M = x.shape[0] * x.shape[1]
    sel = draw(M, K, seed)
    cs = cb.cluster_size.clone()
    expired = cs < thr
    assert expired.any() and (~expired).any(), f"{name}: need expired and live codes"
    assert ((cs - thr).abs() > 1e-4 * thr).all(), f"{name}: a cluster size at the threshold"
    flat = x.reshape(-1, D)
    assert torch.equal(cb.embed[expired], flat[sel][expired]), f"{name}: sel does not reproduce"
    out.update({f"{name}_sel": sel.numpy().astype(np.int32), f"{name}_expired": expired.numpy(),
                f"{name}_ind": ind.numpy().astype(np.int16),
                f"{name}_post_embed": cb.embed.numpy().copy(),
                f"{name}_post_embed_avg": cb.embed_avg.numpy().copy(),
                f"{name}_post_cluster_size": cs.numpy().copy()})
    print(f"{name}: x {tuple(shape)}: {int(expired.sum())} of {K} codes expired")
    return out


def main():
    import types
    ref = types.SimpleNamespace(vq=_load("ref_vq", f"{REF}/models/vq.py"))
    files = {}
    for name, (M, K, D, kind, seed, fn) in CASES.items():
        files.setdefault(fn, {}).update(gen_kmeans(ref, name, M, K, D, kind, seed))
    files["g12_vq_init.npz"].update(gen_expire(ref, "e1", (25, 40, 32), 11))
    files["g12_vq_init.npz"].update(gen_expire(ref, "e2", (5, 8, 32), 11))
    for fn, d in files.items():
        path = os.path.join(OUT, fn)
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        assert size < (1 << 20), f"{fn}: {size} bytes"
        print(f"wrote {fn}: {size} bytes")


if __name__ == "__main__":
    main()
