"""Weights that change between two calls: nothing derived from them may be reused.

Sampling keeps copies of the weights in other layouts -- the LF prior's packed workspace
(`BidirectionalTransformer._eval_ws`, reused by `sample(first=False)`), the captured batch of
`GraphedSampler` (its launches, the convs' PackCache arena), the folded tables `_head_hf_eval`
composes, the running statistics the fused conv + BN eval launches read.  After an optimizer
step or a load_state_dict a stale copy would go unnoticed by tests that sample once from fresh
weights.  Here every result after a change is compared, token for token or bit for bit, with
a deep copy of the model that received the same change and was never sampled before (no
cached workspace), and the conv + BN launches with torch fp64 on the new statistics.

The model is the small bench.JointTrainer(length=64, channels=3) one of test_sampler.py, whose
LF prior takes the fused eval launch (asserted)."""
import copy

import pytest
import torch

from test_dispatch_modes import (SPECS, Ref, check_y, has, inputs, master, reference, rel_l2, rel_max,
                                 run, set_modes)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pristine(cuda):
    """The model as built: never sampled, never changed; the tests work on deep copies."""
    import bench
    tr = bench.JointTrainer(cuda, 1, length=64, channels=3)
    return tr.s2.maskgit.eval()


def _copy(mg):
    c = copy.deepcopy(mg).eval()
    assert not c.transformer_l._eval_ws
    return c


def _priors(mg):
    return list(mg.transformer_l.parameters()) + list(mg.transformer_h.parameters())


def _scale_priors(mg):
    with torch.no_grad():
        for p in _priors(mg):
            p.mul_(1.01)


def _change_decoders(mg):
    """The decoders' BatchNorm running statistics and both codebooks, in place."""
    with torch.no_grad():
        for dec in (mg.decoder_l, mg.decoder_h):
            for mod in dec.modules():
                if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                    mod.running_mean.add_(0.05)
                    mod.running_var.mul_(1.1)
        for vq in (mg.vq_model_l, mg.vq_model_h):
            vq._codebook.embed.mul_(1.02)


def _decode(mg, cuda, seed, num=8):
    from timevqvae.hip import rng
    rng.manual_seed(seed)
    s_l, s_h = mg.iterative_decoding(num=num, device=cuda)
    torch.cuda.synchronize()
    return s_l.clone(), s_h.clone()


def _lf_fused(mg, cuda):
    from timevqvae.hip import xf
    s = torch.zeros((8, mg.num_tokens_l), dtype=torch.int64, device=cuda)
    with torch.no_grad():
        return xf.prior_lf_eval_supported(mg.transformer_l, s)


@pytest.mark.parametrize("how", ["in_place", "load_state_dict"])
def test_eager_sampling_after_weight_change(how, pristine, cuda):
    """iterative_decoding, then every prior parameter changed (in place, or through
    load_state_dict), then iterative_decoding again: token for token what a never-sampled
    copy with the new weights draws from the same seed -- and not what the old weights drew."""
    from timevqvae.hip._native import plan_trace
    mg, fresh = _copy(pristine), _copy(pristine)
    assert _lf_fused(mg, cuda)
    with plan_trace() as tr:
        old = _decode(mg, cuda, 5)
    assert has(tr.lines, "prior_lf_eval_sample") and mg.transformer_l._eval_ws
    if how == "in_place":
        _scale_priors(mg)
        _scale_priors(fresh)
    else:
        donor = _copy(pristine)
        _scale_priors(donor)
        sd = {k: v.clone() for k, v in donor.state_dict().items()}
        mg.load_state_dict(sd)
        fresh.load_state_dict(sd)
    assert _lf_fused(mg, cuda) and _lf_fused(fresh, cuda)
    got = _decode(mg, cuda, 5)
    want = _decode(fresh, cuda, 5)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], old[0]) and not torch.equal(got[1], old[1])


def test_sample_first_true_repacks(pristine, cuda):
    """`sample(first=False)` may reuse the packed weights of the previous call by contract;
    `first=True` after a change may not: it equals the never-sampled copy bit for bit, and its
    logits are the unfused paths' (FUSED_SAMPLE off: the logits launch without a kept
    workspace; PRIOR_FUSED off: the per-op prior) within test_prior_eval.py's 1e-4 rel-L2."""
    from timevqvae.hip import rng, xf
    from timevqvae.models import bidirectional_transformer as bt
    mg, fresh = _copy(pristine), _copy(pristine)
    tf, tf_fresh = mg.transformer_l, fresh.transformer_l
    K = mg.mask_token_ids["lf"]
    g = torch.Generator().manual_seed(3)
    s = torch.randint(0, K, (8, mg.num_tokens_l), generator=g)
    s[torch.rand(s.shape, generator=g) < 0.6] = K
    s = s.to(cuda)
    assert _lf_fused(mg, cuda)

    def draw(t, first):
        rng.manual_seed(4)
        with torch.no_grad():
            out = t.sample(s, mask_id=K, site=7, want_logits=True, first=first)
        torch.cuda.synchronize()
        return [o.clone() for o in out]

    before = draw(tf, True)
    again = draw(tf, False)  # same weights: the reuse the contract allows
    assert all(torch.equal(a, b) for a, b in zip(before, again))
    _scale_priors(mg)
    _scale_priors(fresh)
    got = draw(tf, True)
    want = draw(tf_fresh, True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert rel_l2(got[2], before[2]) > 1e-3  # the change is far outside the bar below
    for flag_owner, flag in ((bt, "FUSED_SAMPLE"), (xf, "PRIOR_FUSED")):
        setattr(flag_owner, flag, False)
        try:
            unfused = draw(tf, True)
        finally:
            setattr(flag_owner, flag, True)
        assert rel_l2(got[2], unfused[2]) < 1e-4, (flag, rel_l2(got[2], unfused[2]))


def test_graphed_sampler_replay_after_weight_change(pristine, cuda):
    """Capture, replay, then change the priors, the decoders' BatchNorm running statistics and
    the codebooks in place: the next replay equals eager decoding of a never-sampled copy with
    the same changes, bit for bit (the pattern of test_graphed_sampler_equals_eager)."""
    from timevqvae.hip import rng
    from timevqvae.utils.sample_utils import GraphedSampler
    mg, fresh = _copy(pristine), _copy(pristine)
    gs = GraphedSampler(mg, 8, cuda)
    rng.manual_seed(7)
    old = [t.clone() for t in gs.sample()]
    for m in (mg, fresh):
        _scale_priors(m)
        _change_decoders(m)
    rng.manual_seed(7)
    got = [t.clone() for t in gs.sample()]
    rng.manual_seed(7)
    with torch.no_grad():
        rng.advance(cuda)
        s_l, s_h = fresh.iterative_decoding(num=8, device=cuda)
        x_l = fresh.decode_token_ind_to_timeseries(s_l, "lf")
        x_h = fresh.decode_token_ind_to_timeseries(s_h, "hf")
        want = [x_l, x_h, x_l + x_h]
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert not torch.equal(got[0], old[0]) and not torch.equal(got[1], old[1])


@pytest.mark.parametrize("name", ["dec", "enc", "res16", "res64", "proj", "ups"])
def test_fused_bn_eval_after_statistics_change(name, cuda):
    """The fused conv + BN eval launch of a decoder block (and of the other blocks), run,
    the running statistics changed in place, run again: the second result is torch fp64 with
    the new statistics (1e-4 of max-abs), far from the first."""
    spec = SPECS[name]
    m = copy.deepcopy(master(name)).to(cuda)
    first = run(name, cuda, False, False, False, m=m)
    assert all(has(first["trace"], k) for k in spec.evalm), first["trace"]
    check_y(spec, first, reference(name, False))
    cpu = copy.deepcopy(master(name))
    for mod in (m, cpu):
        with torch.no_grad():
            for bn in spec.bns(mod):
                bn.running_mean.add_(0.5)
                bn.running_var.mul_(1.7)
    set_modes(spec, cpu, False, False)
    want = spec.ref(Ref(cpu), cpu, *[t.double() for t in inputs(name)]).detach()
    second = run(name, cuda, False, False, False, m=m)
    assert all(has(second["trace"], k) for k in spec.evalm), second["trace"]
    assert rel_max(second["y"], want) < 1e-4, rel_max(second["y"], want)
    assert rel_max(first["y"], want) > 1e-2
