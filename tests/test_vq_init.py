"""VQ codebook health options: k-means initialisation (kmeans_init) and dead-code expiry
(threshold_ema_dead_code > 0) against the reference goldens G12
(tests/golden/make_golden_vq_init.py; reference vq.py:67-106, 170-195, 243).

The goldens carry the rows the reference's generator drew (`sel`), so the parity tests inject
them; the device draw is tested on its own (range, distinctness, spread, redraw per replay).
The generator asserted that no sample of any k-means iteration sits at a near tie (relative
fp64 gap of the two best squared distances >= 1e-5) and that fp32 and fp64 agree on every
bucket, so buckets and bins must be exact here; the means carry the 1e-4 row-relative bound
that test_vq.py uses for `embed`.
"""
import numpy as np
import pytest
import torch

from conftest import golden
from oracle import vq_ref

KM_CASES = ["c1", "c2", "c3", "c4", "c5"]
ITERS = [1, 2, 10]
STATE_KEYS = {"_codebook.initted", "_codebook.cluster_size", "_codebook.embed_avg",
              "_codebook.embed"}
_G = {}


def G():
    if not _G:
        for fn in ("g12_vq_init.npz", "g12_vq_init_c3.npz", "g12_vq_init_c4.npz"):
            with golden(fn) as f:
                _G.update({k: f[k] for k in f.files})
    return _G


def row_rel_err(got, want):
    return float((np.abs(got - want) / np.linalg.norm(want, axis=1, keepdims=True)).max())


# ------------------------------------------------------------------ NumPy restatements
def kmeans_np(x, sel, iters):
    """vq.py:78-106 in fp32 from the drawn rows `sel`: (means, bins, buckets of the last
    assignment)."""
    K = len(sel)
    means = x[sel].copy()
    for _ in range(iters):
        d = ((x[:, None, :] - means[None, :, :]) ** 2).sum(-1, dtype=np.float32)
        buckets = d.argmin(1)  # first index on ties, as max(-d).indices
        bins = np.bincount(buckets, minlength=K)
        sums = np.zeros_like(means)
        np.add.at(sums, buckets, x)
        new = sums / np.maximum(bins, 1)[:, None].astype(np.float32)
        means = np.where((bins == 0)[:, None], means, new)
    return means, bins, buckets


def expire_np(embed, cluster_size, rows, sel, threshold):
    """vq.py:181-195: (embed with the expired codes' rows replaced, expired mask)."""
    expired = cluster_size < np.float32(threshold)
    return np.where(expired[:, None], rows[sel], embed), expired


# ----------------------------------------------------------------------------- CPU
def test_kmeans_init_constructs_like_the_reference():
    from timevqvae.models import VectorQuantize
    vq = VectorQuantize(32, 64, kmeans_init=True, kmeans_iters=10)
    cb = vq._codebook
    assert cb.embed.shape == (64, 32) and not cb.embed.any() and not cb.embed_avg.any()
    assert float(cb.initted) == 0.0 and cb._initted is False
    assert set(vq.state_dict()) == STATE_KEYS
    plain = VectorQuantize(32, 64)
    assert float(plain._codebook.initted) == 1.0 and plain._codebook._initted is True
    assert plain._codebook.embed.any()


def test_dead_code_threshold_constructs():
    from timevqvae.models import VectorQuantize
    from timevqvae.models.vq import EuclideanCodebook
    assert VectorQuantize(32, 64, threshold_ema_dead_code=2)._codebook.threshold_ema_dead_code == 2
    assert EuclideanCodebook(32, 64).threshold_ema_dead_code == 2  # the reference's own default


def test_load_state_dict_refreshes_the_host_flag():
    from timevqvae.models import VectorQuantize
    vq = VectorQuantize(32, 64, kmeans_init=True)
    sd = {k: v.clone() for k, v in VectorQuantize(32, 64).state_dict().items()}
    assert float(sd["_codebook.initted"]) == 1.0
    vq.load_state_dict(sd)
    assert vq._codebook._initted is True and float(vq._codebook.initted) == 1.0
    # an initialised codebook never fits again, whatever its input
    vq._codebook.init_embed_(torch.zeros(8, 32))
    assert torch.equal(vq._codebook.embed, sd["_codebook.embed"])
    sd["_codebook.initted"] = torch.zeros(1)
    vq.load_state_dict(sd)
    assert vq._codebook._initted is False


def test_unsupported_options_still_raise():
    from timevqvae.models import VectorQuantize
    from timevqvae.models.vq import EuclideanCodebook
    with pytest.raises(NotImplementedError):
        EuclideanCodebook(32, 64, learnable_codebook=True)
    with pytest.raises(NotImplementedError):
        EuclideanCodebook(32, 64, emb_dropout=0.1)
    with pytest.raises(NotImplementedError):
        VectorQuantize(32, 64, emb_dropout=0.1)


def test_options_refused_on_several_ranks(monkeypatch):
    """sync_codebook with world_size > 1: both options raise and name themselves; world
    size 1 behaves as a single process."""
    import torch.distributed as dist
    from timevqvae.models import VectorQuantize
    km = VectorQuantize(32, 64, kmeans_init=True, sync_codebook=True)._codebook
    ex = VectorQuantize(32, 64, threshold_ema_dead_code=2, sync_codebook=True)._codebook
    world = [2]
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: world[0])
    with pytest.raises(NotImplementedError, match="kmeans_init"):
        km.init_embed_(torch.zeros(8, 32))
    with pytest.raises(NotImplementedError, match="threshold_ema_dead_code"):
        ex._expire_threshold()
    world[0] = 1
    assert ex._expire_threshold() == 2
    local = VectorQuantize(32, 64, threshold_ema_dead_code=2)._codebook  # no sync_codebook
    world[0] = 2
    assert local._expire_threshold() == 2


@pytest.mark.parametrize("case", KM_CASES)
def test_numpy_kmeans_matches_reference_golden(case):
    g = G()
    x, sel = g[f"{case}_x"], g[f"{case}_sel"]
    for iters in ITERS:
        means, bins, buckets = kmeans_np(x, sel, iters)
        assert (buckets == g[f"{case}_buckets{iters}"]).all()
        assert (bins == g[f"{case}_bins{iters}"]).all()
        assert row_rel_err(means, g[f"{case}_means{iters}"]) < 1e-4
    if case == "c2":
        assert (g["c2_bins10"] == 0).sum() == 3  # the keep-old-mean branch is exercised
    if case == "c5":
        assert (g["c5_bins10"] == 0).sum() == 27 and len(x) < len(sel)


@pytest.mark.parametrize("case", ["e1", "e2"])
def test_numpy_expiry_matches_reference_golden(case):
    g = G()
    x = g[f"{case}_x"].reshape(-1, 32)
    cs, ea, E1, _, _ = vq_ref.ema(x, g[f"{case}_ind"].reshape(-1).astype(np.int64),
                                  g[f"{case}_cluster_size"], g[f"{case}_embed_avg"], decay=0.8)
    np.testing.assert_allclose(cs, g[f"{case}_post_cluster_size"], rtol=1e-5, atol=1e-5)
    E2, expired = expire_np(E1.astype(np.float32), cs.astype(np.float32), x, g[f"{case}_sel"], 2)
    assert (expired == g[f"{case}_expired"]).all() and expired.any() and not expired.all()
    post = g[f"{case}_post_embed"]
    assert (E2[expired] == post[expired]).all()
    assert row_rel_err(E2[~expired], post[~expired]) < 1e-4


# ----------------------------------------------------------------------------- GPU
def _nchw_view(x, B, H, W):
    """The 'b c h w -> b (h w) c' view of an NCHW tensor whose token rows are x's."""
    M, D = x.shape
    t = x.reshape(B, H * W, D).transpose(1, 2).contiguous().reshape(B, D, H, W)
    v = t.flatten(2).transpose(1, 2)
    assert v.stride(2) != 1 and torch.equal(v.reshape(M, D), x)
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("case", KM_CASES)
@pytest.mark.parametrize("iters", ITERS)
def test_hip_kmeans_matches_reference_golden(case, iters, cuda):
    from timevqvae.hip.vq import kmeans_init
    g = G()
    x = torch.from_numpy(g[f"{case}_x"]).to(cuda)
    sel = torch.from_numpy(g[f"{case}_sel"]).to(cuda)
    means, bins = kmeans_init(x, len(sel), iters, sel=sel)
    means2, bins2 = kmeans_init(x, len(sel), iters, sel=sel)
    torch.cuda.synchronize()
    assert bins.dtype == torch.float32
    assert (bins.cpu().numpy() == g[f"{case}_bins{iters}"]).all()
    err = row_rel_err(means.cpu().numpy(), g[f"{case}_means{iters}"])
    print(f"{case} iters {iters}: max row-relative mean error {err:.3g}")
    assert err < 1e-4
    assert torch.equal(means, means2) and torch.equal(bins, bins2)


@pytest.mark.gpu
@pytest.mark.parametrize("case,B,H,W", [("c1", 5, 8, 25), ("c4", 6, 16, 16)])
def test_hip_kmeans_strided_input_is_bitwise_the_same(case, B, H, W, cuda):
    from timevqvae.hip.vq import kmeans_init
    g = G()
    x = torch.from_numpy(g[f"{case}_x"]).to(cuda)
    sel = torch.from_numpy(g[f"{case}_sel"]).to(cuda)
    K = len(sel)
    m0, b0 = kmeans_init(x.reshape(B, H * W, -1), K, 10, sel=sel)
    m1, b1 = kmeans_init(_nchw_view(x, B, H, W), K, 10, sel=sel)
    assert torch.equal(m0, m1) and torch.equal(b0, b1)
    assert (b0.cpu().numpy() == g[f"{case}_bins10"]).all()


@pytest.mark.gpu
def test_hip_kmeans_rejects_unsupported_dim(cuda):
    from timevqvae.hip._native import NativeError
    from timevqvae.hip.vq import kmeans_init
    with pytest.raises(NativeError, match="unsupported codebook dim"):
        kmeans_init(torch.randn(64, 48, device=cuda), 8, 2,
                    sel=torch.arange(8, dtype=torch.int32, device=cuda))


def _buffers(vq):
    cb = vq._codebook
    return cb.embed.clone(), cb.embed_avg.clone(), cb.cluster_size.clone()


def _train_pass(vq, x):
    xg = x.clone().requires_grad_(True)
    q, _, loss, _ = vq(xg)
    (q.square().sum() + loss["loss"].sum()).backward()
    return xg.grad


@pytest.mark.gpu
def test_module_kmeans_init_path(cuda):
    """The first forward fits the codebook and then runs on it: bitwise an explicit
    kmeans_init loaded into a kmeans_init=False module, followed by the same pass."""
    from timevqvae.hip import rng
    from timevqvae.hip.vq import _KMEANS_SITE, draw_rows, kmeans_init
    from timevqvae.models import VectorQuantize
    g = G()
    K, D = 32, 32
    x = torch.from_numpy(g["c1_x"]).to(cuda).reshape(25, 40, D)
    gsel = torch.from_numpy(g["c1_sel"]).to(cuda)

    def twin(sel):
        means, bins = kmeans_init(x, K, 10, sel=sel)
        t = VectorQuantize(D, K).to(cuda).train()
        t._codebook.embed.copy_(means)
        t._codebook.embed_avg.copy_(means)
        t._codebook.cluster_size.copy_(bins)
        return t, means, bins

    # rows injected through init_embed_, then the forward (which must not fit again)
    vq = VectorQuantize(D, K, kmeans_init=True, kmeans_iters=10).to(cuda).train()
    vq._codebook.init_embed_(x, sel=gsel)
    assert float(vq._codebook.initted) == 1.0 and vq._codebook._initted
    assert row_rel_err(vq._codebook.embed.cpu().numpy(), g["c1_means10"]) < 1e-4
    assert (vq._codebook.cluster_size.cpu().numpy() == g["c1_bins10"]).all()
    ref, _, _ = twin(gsel)
    for _ in range(2):  # the second forward does not re-initialise
        ga, gb = _train_pass(vq, x), _train_pass(ref, x)
        assert torch.equal(ga, gb)
        for a, b in zip(_buffers(vq), _buffers(ref)):
            assert torch.equal(a, b)

    # rows drawn on the device by the forward itself, in train and in eval mode
    for train in (True, False):
        vq = VectorQuantize(D, K, kmeans_init=True, kmeans_iters=10).to(cuda).train(train)
        rng.restart_calls()
        sel = draw_rows(x.shape[0] * x.shape[1], K, cuda, offset=_KMEANS_SITE + 1)
        assert len(set(sel.tolist())) == K
        ref, means, bins = twin(sel)
        ref.train(train)
        rng.restart_calls()
        if train:
            _train_pass(vq, x)
            _train_pass(ref, x)
        else:
            q, ind, _, _ = vq(x)
            q2, ind2, _, _ = ref(x)
            assert torch.equal(q, q2) and torch.equal(ind, ind2)
            assert torch.equal(vq._codebook.embed, means)
            assert torch.equal(vq._codebook.cluster_size, bins)
        assert float(vq._codebook.initted) == 1.0 and vq._codebook._initted
        for a, b in zip(_buffers(vq), _buffers(ref)):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_uninitialised_codebook_refuses_capture(cuda, monkeypatch):
    from timevqvae.models import VectorQuantize
    vq = VectorQuantize(32, 32, kmeans_init=True).to(cuda)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="eager"):
        vq._codebook.init_embed_(torch.zeros(64, 32, device=cuda))
    assert not vq._codebook._initted


def _expiry_module(g, case, threshold, cuda):
    from timevqvae.models import VectorQuantize
    vq = VectorQuantize(32, 64, decay=0.8, threshold_ema_dead_code=threshold).to(cuda).train()
    cb = vq._codebook
    cb.embed.copy_(torch.from_numpy(g[f"{case}_embed"]))
    cb.embed_avg.copy_(torch.from_numpy(g[f"{case}_embed_avg"]))
    cb.cluster_size.copy_(torch.from_numpy(g[f"{case}_cluster_size"]))
    return vq


def _expiry_run(g, case, threshold, cuda, mode):
    from timevqvae.hip.vq import deferred_codebook_updates
    vq = _expiry_module(g, case, threshold, cuda)
    vq._codebook.expire_sel = torch.from_numpy(g[f"{case}_sel"]).to(cuda)
    x = torch.from_numpy(g[f"{case}_x"]).to(cuda)
    if mode == "nchw":
        B, N, D = x.shape
        H = 5 if N % 5 == 0 else 2
        x = _nchw_view(x.reshape(-1, D), B, H, N // H)
    if mode == "deferred":
        with deferred_codebook_updates() as pend:
            _train_pass(vq, x)
        assert len(pend) == 1
        for u in pend:
            u.reduce()
            u.apply()
    else:
        _train_pass(vq, x)
    torch.cuda.synchronize()
    return _buffers(vq)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["e1", "e2"])
def test_hip_expiry_matches_reference_golden(case, cuda):
    g = G()
    thr = 2
    xf = g[f"{case}_x"].reshape(-1, 32)
    sel, want = g[f"{case}_sel"], g[f"{case}_expired"]
    base = _expiry_run(g, case, 0, cuda, "immediate")  # the identical module with expiry off
    imm = _expiry_run(g, case, thr, cuda, "immediate")
    for mode, got in (("immediate", imm), ("deferred", _expiry_run(g, case, thr, cuda, "deferred")),
                      ("nchw", _expiry_run(g, case, thr, cuda, "nchw"))):
        embed, embed_avg, cs = (t.cpu().numpy() for t in got)
        expired = cs < thr
        assert (expired == want).all(), mode
        assert (embed[expired] == xf[sel][expired]).all(), mode  # bitwise the selected rows
        assert (embed[~expired] == base[0].cpu().numpy()[~expired]).all(), mode
        assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2]), mode
        np.testing.assert_allclose(cs, g[f"{case}_post_cluster_size"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(embed_avg, g[f"{case}_post_embed_avg"], rtol=1e-4, atol=1e-5)
        post = g[f"{case}_post_embed"]
        assert (embed[expired] == post[expired]).all(), mode
        assert row_rel_err(embed[~expired], post[~expired]) < 1e-4, mode
        for a, b in zip(got, imm):  # deferred reduce() + apply(), and the NCHW view: bitwise
            assert torch.equal(a, b), mode


@pytest.mark.gpu
def test_expire_function_and_module_methods(cuda):
    """hip.vq.expire / EuclideanCodebook.expire_codes_ / replace on their own: no expired
    code writes nothing, the count comes back, only embed changes."""
    from timevqvae.hip.vq import expire
    from timevqvae.models.vq import EuclideanCodebook
    g = G()
    x = torch.from_numpy(g["e1_x"]).to(cuda)
    xf = x.reshape(-1, 32)
    sel = torch.from_numpy(g["e1_sel"]).to(cuda)
    cb = EuclideanCodebook(32, 64).to(cuda)
    E0 = cb.embed.clone()
    cb.cluster_size.fill_(5.0)
    n = torch.full((1,), -1, dtype=torch.int32, device=cuda)
    expire(x, cb.embed, cb.cluster_size, 2, sel=sel, n_expired=n)
    assert torch.equal(cb.embed, E0) and int(n) == 0
    cb.cluster_size[::3] = 0.5
    ea0 = cb.embed_avg.clone()
    expire(x, cb.embed, cb.cluster_size, 2, sel=sel, n_expired=n)
    mask = cb.cluster_size < 2
    assert int(n) == int(mask.sum()) == 22
    assert torch.equal(cb.embed, torch.where(mask[:, None], xf[sel.long()], E0))
    assert torch.equal(cb.embed_avg, ea0)
    cb.embed.copy_(E0)
    cb.expire_codes_(x, sel=sel)
    assert torch.equal(cb.embed, torch.where(mask[:, None], xf[sel.long()], E0))
    cb.embed.copy_(E0)
    cb.replace(xf, ~mask, sel=sel)
    assert torch.equal(cb.embed, torch.where(~mask[:, None], xf[sel.long()], E0))
    # the device draw: every replaced row is one of x's rows, all different (M >= K)
    cb.embed.copy_(E0)
    cb.expire_codes_(x)
    rows = [int((xf == cb.embed[k]).all(1).nonzero()[0]) for k in mask.nonzero().flatten().tolist()]
    assert len(set(rows)) == len(rows)
    assert torch.equal(cb.embed[~mask], E0[~mask])


@pytest.mark.gpu
def test_device_row_draw(cuda):
    from timevqvae.hip import rng
    from timevqvae.hip.vq import draw_rows
    seed = rng.seed_tensor(cuda)
    keep = seed.clone()
    try:
        seed.fill_(0x5EED)
        draws = torch.stack([draw_rows(64, 32, cuda, offset=o) for o in range(1, 201)]).cpu().numpy()
        assert draws.min() >= 0 and draws.max() < 64
        assert all(len(set(d)) == 32 for d in draws)  # M >= K: distinct
        hits = np.bincount(draws.reshape(-1), minlength=64)
        # Binomial(200, 1/2): mean 100, sigma 7.07; 5 sigma
        assert hits.min() >= 64 and hits.max() <= 136, (hits.min(), hits.max())
        assert len(set(draws[:, 0])) >= 50  # 61.3 expected of 64
        rep = torch.stack([draw_rows(40, 64, cuda, offset=o) for o in range(1, 11)]).cpu().numpy()
        assert rep.min() >= 0 and rep.max() < 40
        assert all(len(set(d)) >= 24 for d in rep)  # with replacement: 32.1 expected
        a, b = draw_rows(64, 32, cuda, offset=7), draw_rows(64, 32, cuda, offset=7)
        assert torch.equal(a, b) and (a.cpu().numpy() == draws[6]).all()
        seed.add_(1)  # another seed, another draw
        assert not torch.equal(a, draw_rows(64, 32, cuda, offset=7))
        big = draw_rows(100000, 512, cuda, offset=3).cpu().numpy()
        assert big.min() >= 0 and big.max() < 100000 and len(set(big)) == 512
        one = draw_rows(1, 1, cuda, offset=3)
        assert int(one) == 0
    finally:
        seed.copy_(keep)


@pytest.mark.gpu
def test_graph_replay_with_expiry_matches_eager(cuda):
    """A training step with dead-code expiry, captured in a StepGraph: replays equal eager
    steps bit for bit (the expiry's rows come from the device seed, advanced before every
    step), and consecutive replays pick different rows."""
    from timevqvae.hip import rng
    from timevqvae.hip.graph import StepGraph
    from timevqvae.models import VectorQuantize
    K, D = 64, 32
    gen = torch.Generator().manual_seed(9)
    x0 = torch.randn(4, 20, D, generator=gen)  # 80 rows for 64 codes: most codes stay dead
    E0 = torch.randn(K, D, generator=gen)

    def make():
        rng.manual_seed(77)
        vq = VectorQuantize(D, K, threshold_ema_dead_code=2).to(cuda).train()
        vq._codebook.embed.copy_(E0)
        vq._codebook.embed_avg.copy_(E0)
        x = x0.to(cuda).requires_grad_(True)

        def seg():
            rng.restart_calls()  # host state: the captured step numbers its calls as an eager one
            x.grad = None
            q, _, loss, _ = vq(x)
            (q.square().sum() + loss["loss"].sum()).backward()
            return loss["loss"]

        return vq, x, StepGraph([seg], before=lambda: rng.advance(cuda))

    def chosen(vq, x):
        """(expired mask, the row of x every code's embedding equals, -1 if none)."""
        xf = x.detach().reshape(-1, D)
        eq = (vq._codebook.embed[:, None, :] == xf[None, :, :]).all(-1)
        row = torch.where(eq.any(1), eq.float().argmax(1), torch.full((K,), -1, device=cuda))
        return (vq._codebook.cluster_size < 2).cpu(), row.cpu()

    ve, xe, sge = make()
    for _ in range(4):
        sge._eager()
    torch.cuda.synchronize()
    eager = _buffers(ve)

    vg, xg, sgg = make()
    sgg.capture()  # 2 eager warm-up steps
    sgg.replay()
    torch.cuda.synchronize()
    m1, r1 = chosen(vg, xg)
    sgg.replay()
    torch.cuda.synchronize()
    m2, r2 = chosen(vg, xg)
    for a, b in zip(eager, _buffers(vg)):
        assert torch.equal(a, b)
    both = m1 & m2
    assert both.sum() >= 8, "both replays must expire codes"
    assert (r1[both] >= 0).all() and (r2[both] >= 0).all()
    assert (r1[both] != r2[both]).any(), "a replay must redraw its rows"
