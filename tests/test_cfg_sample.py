"""Classifier-free guidance inside the fused sampling launches (maskgit.py:136-153:
logits_null + cfg_scale * (logits - logits_null)): tvq_prior_lf_eval_sample_cfg (the LF
prior, csrc/tvq_prior_eval.hip), tvq_tied_logits_sample_cfg (the HF prior's head,
csrc/tvq_sample.hip) and their routing through BidirectionalTransformer.sample /
MaskGIT.sample_tokens / iterative_decoding / GraphedSampler.  Each guided kernel runs the
unguided kernel's draw body with two B operands (pe_draw / tls_body with NB = 2), so the cases
here and in test_prior_eval / test_sampler cover one tile loop from both sides.

Tolerances.  With s the scale, w(s) = |1 - s| + |s| is how the mix scales an error of its two
inputs.  Two launches of the LF kernel agree within 1e-6 of the logit scale
(test_prior_eval.test_fused_prior_draw), the HF head's logits are within 1e-5 of the fp64
ones (test_sampler.test_tied_logits_sample_vs_oracle); the mixes are held to w(s) times
those.  Against the oracle and the unfused path: 1e-4 relative, the project's parity bar.
The draw is exact on the returned logits, p(sampled) within 2e-6 relative."""
import pytest
import torch

from conftest import golden
from oracle import tvq_oracle as O
from test_prior_eval import _prior, rel
from test_sampler import _gumbel, _maskgit

pytestmark = pytest.mark.gpu


def _w(s):
    return abs(1.0 - s) + abs(s)


def _p_close(got, want, tol=2e-6):
    got, want = got.double().cpu(), want.double().cpu()
    return float(((got - want).abs() / want).max()) < tol


@pytest.mark.parametrize("depth,K,n,B,sc", [(2, 70, 7, 9, 2.0), (4, 512, 24, 37, 2.0),
                                            (1, 100, 7, 5, -0.5), (2, 32, 24, 3, 0.0)])
def test_lf_guided_draw(depth, K, n, B, sc, cuda):
    """K = 70: three code tiles (uneven split over the two waves, ragged last tile); K = 32:
    one tile, the second wave has no head tile."""
    from timevqvae.hip import rng, xf
    from timevqvae.hip._native import plan_trace
    from timevqvae.hip.sample import maskgit_sample
    m, sd = _prior(cuda, depth, K, n)
    gen = torch.Generator().manual_seed(5)
    s = torch.randint(0, K, (B, n), generator=gen)
    s[torch.rand(B, n, generator=gen) < 0.6] = K  # mask id K: drawn; the rest kept
    y = torch.randint(0, 5, (B, 1), generator=gen)
    gum = _gumbel((B, n, K), gen)
    sg, yg, gg = s.to(cuda), y.to(cuda), gum.to(cuda)
    with torch.no_grad(), plan_trace() as tr:
        sampled, selp, lg = xf.prior_lf_eval_sample(m, sg, yg, K, gumbel=gg, want_logits=True,
                                                    cfg_scale=sc)
        torch.cuda.synchronize()
    assert tr.has("prior_lf_eval_sample_cfg")
    with torch.no_grad():
        sc_c, pc_c, lc = xf.prior_lf_eval_sample(m, sg, yg, K, gumbel=gg, want_logits=True)
        _, _, ln = xf.prior_lf_eval_sample(m, sg, None, K, gumbel=gg, want_logits=True)
        torch.cuda.synchronize()
    # the mix of the unguided launches' logits
    lcd, lnd = lc.double().cpu(), ln.double().cpu()
    err = float((lg.double().cpu() - (lnd + sc * (lcd - lnd))).abs().max())
    bound = _w(sc) * 1e-6 * max(float(lcd.abs().max()), float(lnd.abs().max()))
    print(f"lf mix vs unguided launches: {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # the oracle's mix, formed in fp32
    rc = O.transformer_forward(O.Ctx(False), sd, "lf", s, None, y, K, 2, depth)
    rn = O.transformer_forward(O.Ctx(False), sd, "lf", s, None, torch.full((B, 1), 5), K, 2, depth)
    ref = rn.float() + sc * (rc.float() - rn.float())
    print(f"lf mix vs oracle: rel {rel(lg, ref):.3e}")
    assert rel(lg, ref) < 1e-4
    # the draw on the returned logits: exact; p(sampled); known tokens kept
    want, sel = O.race_sample(lg.cpu(), s, K, gum)
    assert torch.equal(sampled.cpu(), want)
    unk = s == K
    assert torch.isinf(selp.cpu()[~unk]).all()
    assert _p_close(selp.cpu()[unk], sel[unk])
    # device noise: what maskgit_sample draws from the returned logits at the same offset
    with torch.no_grad():
        rng.manual_seed(8)
        a, pa, lg2 = xf.prior_lf_eval_sample(m, sg, yg, K, site=3, want_logits=True, cfg_scale=sc)
        rng.manual_seed(8)
        b, pb = maskgit_sample(lg2, sg, K, site=3)
        # the product form (no logits copy): the same bits
        rng.manual_seed(8)
        c, pc = xf.prior_lf_eval_sample(m, sg, yg, K, site=3, cfg_scale=sc)
        torch.cuda.synchronize()
    assert torch.equal(a, b)
    fin = torch.isfinite(pb)
    assert _p_close(pa[fin], pb[fin])
    assert torch.equal(c, a) and torch.equal(pc, pa)
    # one workspace, packed by the unguided entry, read by the guided one and back
    with torch.no_grad():
        ws = xf.prior_lf_eval_workspace(m, sg)
        r1 = xf.prior_lf_eval_sample(m, sg, yg, K, gumbel=gg, want_logits=True, ws=ws, ready=False)
        r2 = xf.prior_lf_eval_sample(m, sg, yg, K, gumbel=gg, want_logits=True, ws=ws, ready=True,
                                     cfg_scale=sc)
        r3 = xf.prior_lf_eval_sample(m, sg, yg, K, gumbel=gg, want_logits=True, ws=ws, ready=True)
        torch.cuda.synchronize()
    for got, fresh in ((r1, (sc_c, pc_c, lc)), (r2, (sampled, selp, lg)), (r3, (sc_c, pc_c, lc))):
        for g_, f_ in zip(got, fresh):
            assert torch.equal(g_, f_)


@pytest.mark.parametrize("B,n,D,K,sc", [(3, 7, 64, 33, 2.0), (5, 13, 128, 100, 0.0),
                                        (9, 96, 128, 512, 3.0), (2, 5, 64, 20, 2.0)])
def test_hf_guided_draw(B, n, D, K, sc, cuda):
    from timevqvae.hip import rng
    from timevqvae.hip._native import plan_trace
    from timevqvae.hip.sample import maskgit_sample, tied_logits_sample_cfg
    g = torch.Generator().manual_seed(B + n + D + K)
    hc = torch.randn(B, n, D, generator=g)
    hn = torch.randn(B, n, D, generator=g)
    W = torch.randn(K + 1, D, generator=g) * D ** -0.5
    bias = torch.randn(n, K + 1, generator=g) * 0.3
    mask_id = K
    s = torch.randint(0, K, (B, n), generator=g)
    s[torch.rand(B, n, generator=g) < 0.7] = mask_id
    gum = _gumbel((B, n, K), g)
    dev = [t.to(cuda) for t in (hc, hn, W, bias)]
    sg, gg = s.to(cuda), gum.to(cuda)
    with plan_trace() as tr:
        sampled, selp, lg = tied_logits_sample_cfg(*dev, K, sg, mask_id, sc, gumbel=gg,
                                                   want_logits=True)
        torch.cuda.synchronize()
    assert tr.has("tied_logits_sample_cfg D=")
    l_c = hc.double() @ W[:K].double().t() + bias[:, :K].double()
    l_n = hn.double() @ W[:K].double().t() + bias[:, :K].double()
    lcpu = lg.cpu()
    err = float((lcpu.double() - (l_n + sc * (l_c - l_n))).abs().max())
    bound = _w(sc) * 1e-5 * max(float(l_c.abs().max()), float(l_n.abs().max()))
    print(f"hf mix vs fp64: {err:.3e} (bound {bound:.3e})")
    assert err < bound
    want, sel = O.race_sample(lcpu, s, mask_id, gum)
    assert torch.equal(sampled.cpu(), want)
    known = s != mask_id
    assert torch.equal(sampled.cpu()[known], s[known])
    assert torch.isinf(selp.cpu()[known]).all()
    assert _p_close(selp.cpu()[~known], sel[~known])
    s2, p2 = maskgit_sample(lg, sg, mask_id, gumbel=gg)
    assert torch.equal(s2, sampled)
    assert _p_close(selp.cpu()[~known], p2.cpu()[~known])
    rng.manual_seed(4)
    a, pa, lg2 = tied_logits_sample_cfg(*dev, K, sg, mask_id, sc, site=7, want_logits=True)
    rng.manual_seed(4)
    b, pb = maskgit_sample(lg2, sg, mask_id, site=7)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    fin = torch.isfinite(pb)
    assert _p_close(pa[fin], pb[fin])


@pytest.fixture(scope="module")
def bench_maskgit(cuda):
    """The bench's MaskGIT (LF width 128, HF head dim 128), shared: the tests set cfg_scale
    and restore it."""
    return _maskgit(cuda)


def _module_inputs(mg, B, cuda, seed=21):
    g = torch.Generator().manual_seed(seed)
    K_l, K_h = mg.mask_token_ids["lf"], mg.mask_token_ids["hf"]
    s_l = torch.randint(0, K_l, (B, mg.num_tokens_l), generator=g)
    s_lm = s_l.clone()
    s_lm[torch.rand(s_l.shape, generator=g) < 0.6] = K_l
    s_h = torch.randint(0, K_h, (B, mg.num_tokens_h), generator=g)
    s_h[torch.rand(s_h.shape, generator=g) < 0.6] = K_h
    y = torch.randint(0, 5, (B, 1), generator=g)
    return {"lf": (K_l, (s_lm.to(cuda),)), "hf": (K_h, (s_l.to(cuda), s_h.to(cuda)))}, y.to(cuda), g


FUSED_LINE = {"lf": "prior_lf_eval_sample_cfg B=", "hf": "tied_logits_sample_cfg D="}
PLAIN_LINE = {"lf": "prior_lf_eval_sample B=", "hf": "tied_logits_sample D="}


@pytest.mark.parametrize("kind", ["lf", "hf"])
def test_sample_tokens_guided_fused(kind, bench_maskgit, cuda):
    from timevqvae.hip._native import plan_trace
    from timevqvae.models import bidirectional_transformer as bt
    mg = bench_maskgit
    tf = mg.transformer_l if kind == "lf" else mg.transformer_h
    inputs, y, g = _module_inputs(mg, 6, cuda)
    mask_id, s_in = inputs[kind]
    K = mask_id
    gum = _gumbel(tuple(s_in[-1].shape) + (K,), g)
    gg = gum.to(cuda)
    old = mg.cfg_scale
    try:
        mg.cfg_scale = 2.0
        with torch.no_grad(), plan_trace() as tr:
            sampled, selp, lg = mg.sample_tokens(tf, y, mask_id, *s_in, gumbel=gg,
                                                 want_logits=True)
            torch.cuda.synchronize()
        assert tr.has(FUSED_LINE[kind]) and not tr.has(PLAIN_LINE[kind]), tr.lines
        bt.FUSED_SAMPLE = False
        try:
            with torch.no_grad(), plan_trace() as tr0:
                s0, p0, lg0 = mg.sample_tokens(tf, y, mask_id, *s_in, gumbel=gg,
                                               want_logits=True)
                torch.cuda.synchronize()
        finally:
            bt.FUSED_SAMPLE = True
        assert not tr0.has(FUSED_LINE[kind]) and not tr0.has(PLAIN_LINE[kind])
        print(f"{kind} fused vs unfused guided logits: rel {rel(lg, lg0):.3e}")
        assert rel(lg, lg0) < 1e-4
        want, _ = O.race_sample(lg.cpu(), s_in[-1].cpu(), mask_id, gum)
        assert torch.equal(sampled.cpu(), want)
        # the two paths draw the same code wherever the unfused race is decided by more than
        # the fp32 reassociation noise (1e-4 of the row's logit scale)
        l0 = lg0.double().cpu()
        top2 = torch.topk(l0 + gum.double(), 2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-4 * l0.abs().amax(-1)
        agree = sampled.cpu() == s0.cpu()
        assert bool(agree[clear].all()), int((~agree & clear).sum())
        assert float(clear.float().mean()) >= 0.99
        # no guidance: the launches of the tree before guidance
        for scale, cls in ((1.0, y), (2.0, None)):
            mg.cfg_scale = scale
            with torch.no_grad(), plan_trace() as tr1:
                mg.sample_tokens(tf, cls, mask_id, *s_in, gumbel=gg)
                torch.cuda.synchronize()
            assert tr1.has(PLAIN_LINE[kind]) and not tr1.has(FUSED_LINE[kind]), tr1.lines
    finally:
        mg.cfg_scale = old


def test_guided_fallback_is_the_reference(cuda):
    """The golden MaskGIT's priors have tok_emb dim 32: neither guided kernel applies, and
    sample_tokens draws from masked_prediction's logits, the reference's own
    (test_stage2_golden.test_masked_prediction_cfg_vs_reference)."""
    from test_stage2_golden import _maskgit as golden_maskgit
    from timevqvae.hip._native import plan_trace
    g = golden("g9_stage2.npz")
    mg = golden_maskgit(cuda).eval()
    mg.cfg_scale = 2.0
    with torch.no_grad():
        for k in g:
            if k.startswith("mg_post/"):
                name, kk = k[len("mg_post/"):].split(".", 1)
                getattr(mg, name).state_dict()[kk].copy_(torch.from_numpy(g[k]))
    y = torch.from_numpy(g["mg_y"]).to(cuda)
    sl, sh = torch.from_numpy(g["cfg_s_l_M"]).to(cuda), torch.from_numpy(g["cfg_s_h_M"]).to(cuda)
    with torch.no_grad(), plan_trace() as tr:
        _, _, ll = mg.sample_tokens(mg.transformer_l, y, mg.mask_token_ids["lf"], sl,
                                    want_logits=True)
        _, _, lh = mg.sample_tokens(mg.transformer_h, y, mg.mask_token_ids["hf"], sl, sh,
                                    want_logits=True)
        torch.cuda.synchronize()
    assert not tr.has("prior_lf_eval_sample_cfg") and not tr.has("tied_logits_sample_cfg")
    assert rel(ll, torch.from_numpy(g["cfg_logits_l"])) < 1e-4
    assert rel(lh, torch.from_numpy(g["cfg_logits_h"])) < 1e-4
    # the transformer's own draw has no guided form here and says so
    assert not mg.transformer_l.guided_sample_supported(sl)
    with torch.no_grad(), pytest.raises(ValueError):
        mg.transformer_l.sample(sl, class_condition=y, mask_id=mg.mask_token_ids["lf"],
                                cfg_scale=2.0)


def test_guided_decode_eager_and_captured(bench_maskgit, cuda):
    """The whole guided decode: reproducible under one seed, 10 LF + 1 HF guided launches,
    and a GraphedSampler replay equal to the eager batch from the same seed."""
    from timevqvae.hip import rng
    from timevqvae.hip._native import plan_trace
    from timevqvae.utils.sample_utils import GraphedSampler
    mg = bench_maskgit
    old = mg.cfg_scale
    try:
        mg.cfg_scale = 2.0
        rng.manual_seed(5)
        with plan_trace() as tr:
            s_l, s_h = mg.iterative_decoding(num=48, device=cuda, class_index=1)
            torch.cuda.synchronize()
        rng.manual_seed(5)
        s_l2, s_h2 = mg.iterative_decoding(num=48, device=cuda, class_index=1)
        assert torch.equal(s_l, s_l2) and torch.equal(s_h, s_h2)
        assert int(s_l.max()) < mg.mask_token_ids["lf"] and int(s_h.max()) < mg.mask_token_ids["hf"]
        assert len(tr.has(FUSED_LINE["lf"])) == mg.T["lf"] == 10
        assert len(tr.has(FUSED_LINE["hf"])) == mg.T["hf"] == 1
        assert not tr.has(PLAIN_LINE["lf"]) and not tr.has(PLAIN_LINE["hf"])
        gs = GraphedSampler(mg, 48, cuda, class_index=1)
        rng.manual_seed(7)
        got = [t.clone() for t in gs.sample()]
        again = [t.clone() for t in gs.sample()]
        rng.manual_seed(7)
        with torch.no_grad():
            rng.advance(cuda)
            e_l, e_h = mg.iterative_decoding(num=48, device=cuda, class_index=1)
            x_l = mg.decode_token_ind_to_timeseries(e_l, "lf")
            x_h = mg.decode_token_ind_to_timeseries(e_h, "hf")
        for g_, w_ in zip(got, [x_l, x_h, x_l + x_h]):
            assert torch.equal(g_, w_)
        assert not torch.equal(again[2], got[2])
    finally:
        mg.cfg_scale = old


def test_guided_entries_check_arguments(cuda):
    """cls_idx = NULL, a misaligned h_null and D = 48 are refused before any launch."""
    from timevqvae.hip import xf
    from timevqvae.hip._native import NativeError, call, plan_trace, ptr, stream_ptr, value
    m, _ = _prior(cuda, 1, 64, 7)
    K, B, n = 64, 2, 7
    s = torch.full((B, n), K, dtype=torch.int64, device=cuda)
    s, cls, arr, depth, K, ws = xf._prior_lf_args(m, s, None)
    assert cls is None
    gum = torch.zeros(B, n, K, device=cuda)
    sampled = torch.full((B, n), -1, dtype=torch.int64, device=cuda)
    selp = torch.full((B, n), -1.0, device=cuda)
    with plan_trace() as tr:
        with pytest.raises(NativeError):
            call("tvq_prior_lf_eval_sample_cfg", ptr(s), B, n, s.stride(0), None, m.n_classes, 128,
                 arr, depth, K, 1e-12, 2.0, K, ptr(gum), None, 0, ptr(sampled), ptr(selp), None,
                 ptr(ws), 0, stream_ptr())
        with pytest.raises(NativeError):
            call("tvq_prior_lf_eval_sample_cfg", ptr(s), B, n, s.stride(0),
                 ptr(torch.zeros(B, dtype=torch.int64, device=cuda)), m.n_classes, 128, arr, depth,
                 K, 1e-12, float("nan"), K, ptr(gum), None, 0, ptr(sampled), ptr(selp), None,
                 ptr(ws), 0, stream_ptr())
        for D, shift in ((64, 1), (48, 0)):
            M = B * n
            buf = torch.zeros(2 * M * D + 4, device=cuda)
            hc = buf[:M * D]
            hn = buf[M * D + shift:2 * M * D + shift]  # shift 1: 4 bytes off the alignment
            W = torch.zeros(K + 1, D, device=cuda)
            bias = torch.zeros(n, K + 1, device=cuda)
            nbytes = value("tvq_tied_logits_sample_workspace", K, 64, n)
            tws = torch.empty(nbytes // 4, device=cuda)
            with pytest.raises(NativeError):
                call("tvq_tied_logits_sample_cfg", ptr(hc), ptr(hn), M, D, ptr(W), K, ptr(bias), n,
                     bias.stride(0), 2.0, ptr(s), K, ptr(gum), None, 0, ptr(sampled), ptr(selp),
                     None, ptr(tws), stream_ptr())
        torch.cuda.synchronize()
    assert not tr.lines, tr.lines
    assert bool((sampled == -1).all()) and bool((selp == -1.0).all())
