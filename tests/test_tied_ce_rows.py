"""The priors' loss head on the masked tokens only (tvq_masked_rows, tvq_tied_logits_ce on the
row list, tvq_tied_ce_grads on the compact rows; bidirectional_transformer._TiedLogitsCE), at
the smallest shapes that reach each edge of the row list: a ragged last 16-row group, one
16-code tile per wave, every token masked (the whole worst-case grid runs), exactly one, 16
and 17 masked tokens, a position masked in no sample (an empty segment) with a sample masked
at every other position, and a wholly masked sample.

Tolerances are those of tests/test_tied_ce.py (fp32 sums in another order): against this
library's unfused chain loss 1e-6, gradients 1e-5; against torch fp64 autograd of the
reference formula loss 1e-5, gradients 1e-4."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rel(a, r):
    return float((a.double() - r.double()).abs().max() / r.double().abs().max().clamp_min(1e-30))


def _exactly(B, n, count, g):
    keep = torch.ones(B * n, dtype=torch.bool)
    keep[torch.randperm(B * n, generator=g)[:count]] = False
    return keep.reshape(B, n)


def _mask(kind, B, n, g):
    if kind == "ragged":  # a masked count that is no multiple of 16
        keep = torch.rand(B, n, generator=g) >= 0.36
        keep[0, 0] = False
        if int((~keep).sum()) % 16 == 0:
            keep[0, 1] = ~keep[0, 1]
        return keep
    if kind == "random":
        keep = torch.rand(B, n, generator=g) >= 0.36
        keep[0, 0] = False
        return keep
    if kind == "all":
        return torch.zeros(B, n, dtype=torch.bool)
    if kind in ("one", "sixteen", "seventeen"):
        return _exactly(B, n, {"one": 1, "sixteen": 16, "seventeen": 17}[kind], g)
    keep = torch.rand(B, n, generator=g) >= 0.36
    if kind == "empty_segment":  # position 5 masked in no sample, sample 3 masked everywhere else
        keep[3, :] = False
        keep[:, 5] = True
    else:  # "full_sample": sample 3 wholly masked
        keep[3, :] = False
    return keep


CASES = [
    (3, 97, 128, "ragged"),
    (7, 24, 64, "random"),
    (16, 24, 512, "all"),
    (2, 5, 64, "one"),
    (7, 24, 64, "sixteen"),
    (7, 24, 64, "seventeen"),
    (7, 24, 64, "empty_segment"),
    (7, 24, 64, "full_sample"),
]
_cache = {}


def _inputs(B, n, K, kind):
    """The case's host inputs and its fp64 reference, made once."""
    key = (B, n, K, kind)
    if key not in _cache:
        g = torch.Generator().manual_seed(B * n + K + len(kind))
        h = torch.randn(B, n, 128, generator=g)
        W = torch.randn(K + 1, 128, generator=g) / 128 ** 0.5 * 3
        bias = torch.randn(n, K + 1, generator=g) * 0.2
        tgt = torch.randint(0, K, (B, n), generator=g)
        keep = _mask(kind, B, n, g)
        hr = h.double().requires_grad_(True)
        Wr = W.double().requires_grad_(True)
        br = bias.double().requires_grad_(True)
        lr = F.cross_entropy((hr @ Wr[:K].t() + br[:, :K])[~keep], tgt[~keep])
        lr.backward()
        _cache[key] = (h, W, bias, tgt, keep, (lr.detach(), hr.grad, Wr.grad, br.grad))
    return _cache[key]


def _run(h, W, bias, tgt, keep, K, cuda, fused=True):
    from timevqvae.hip.xf import masked_cross_entropy
    from timevqvae.models.bidirectional_transformer import _TiedLogits, tied_logits_ce
    one = torch.ones((), device=cuda)
    hd = h.to(cuda).requires_grad_(True)
    Wd = W.to(cuda).requires_grad_(True)
    bd = bias.to(cuda).requires_grad_(True)
    if fused:
        loss = tied_logits_ce(hd, Wd, bd, K, tgt.to(cuda), keep.to(cuda), one)
    else:
        loss = masked_cross_entropy(_TiedLogits.apply(hd, Wd, bd, K), tgt.to(cuda), keep.to(cuda))
    torch.autograd.backward(loss, one)
    torch.cuda.synchronize()
    return loss.detach().cpu(), hd.grad.cpu(), Wd.grad.cpu(), bd.grad.cpu()


@pytest.mark.parametrize("B,n,K,kind", CASES)
def test_rows_vs_unfused_and_fp64(B, n, K, kind, cuda):
    h, W, bias, tgt, keep, ref = _inputs(B, n, K, kind)
    cnt = int((~keep).sum())
    assert {"ragged": cnt % 16 != 0, "all": cnt == B * n, "one": cnt == 1, "sixteen": cnt == 16,
            "seventeen": cnt == 17}.get(kind, True)
    l1, gh1, gW1, gb1 = _run(h, W, bias, tgt, keep, K, cuda)
    l2, gh2, gW2, gb2 = _run(h, W, bias, tgt, keep, K, cuda, fused=False)
    assert _rel(l1, l2) < 1e-6
    assert _rel(gh1, gh2) < 1e-5
    assert _rel(gW1, gW2) < 1e-5
    assert _rel(gb1, gb2) < 1e-5
    lr, ghr, gWr, gbr = ref
    assert _rel(l1, lr) < 1e-5
    assert _rel(gh1, ghr) < 1e-4
    assert _rel(gW1, gWr) < 1e-4
    assert _rel(gb1, gbr) < 1e-4
    assert torch.equal(gW1[K:], torch.zeros_like(gW1[K:]))  # the mask-token row
    assert torch.equal(gh1[keep], torch.zeros_like(gh1[keep]))  # kept tokens: exact zeros
    assert torch.equal(gb1[:, K:], torch.zeros_like(gb1[:, K:]))
    # a second run on the same inputs: bitwise the same
    for a, b in zip((l1, gh1, gW1, gb1), _run(h, W, bias, tgt, keep, K, cuda)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,n,K,kind", [c for c in CASES
                                        if c[3] in ("ragged", "all", "one", "empty_segment")])
def test_row_list_exact(B, n, K, kind, cuda):
    """rows = the masked token ids b n + pos ordered by position, then by sample; pos_off = the
    positions' first list indices, pos_off[n] = the masked count."""
    from timevqvae.hip._native import call, ptr, stream_ptr
    keep = _inputs(B, n, K, kind)[4]
    kd = keep.to(cuda)
    rows = torch.full((B * n,), -1, device=cuda, dtype=torch.int32)
    pos_off = torch.full((n + 1,), -1, device=cuda, dtype=torch.int32)
    call("tvq_masked_rows", ptr(kd), B, n, ptr(rows), ptr(pos_off), stream_ptr())
    torch.cuda.synchronize()
    nz = torch.nonzero(~keep.t())  # (pos, b) in position-major order
    want = (nz[:, 1] * n + nz[:, 0]).to(torch.int32)
    cnt = want.numel()
    assert torch.equal(rows.cpu()[:cnt], want)
    assert torch.equal(rows.cpu()[cnt:], torch.full((B * n - cnt,), -1, dtype=torch.int32))
    off = torch.zeros(n + 1, dtype=torch.int32)
    off[1:] = torch.cumsum((~keep).sum(0), 0).to(torch.int32)
    assert torch.equal(pos_off.cpu(), off)
    if kind == "empty_segment":
        assert int(off[6] - off[5]) == 0


def test_graph_replay_serves_another_mask(cuda):
    """Forward and backward captured once on (8, 24, 64); `keep` and `target` overwritten in
    place with a mask of another count; the replay equals an eager run on the new mask bitwise
    (the masked count never reaches the host)."""
    from timevqvae.hip.graph import StepGraph
    from timevqvae.models.bidirectional_transformer import tied_logits_ce
    B, n, K = 8, 24, 64
    g = torch.Generator().manual_seed(11)
    h = torch.randn(B, n, 128, generator=g).to(cuda).requires_grad_(True)
    W = (torch.randn(K + 1, 128, generator=g) / 128 ** 0.5 * 3).to(cuda).requires_grad_(True)
    bias = (torch.randn(n, K + 1, generator=g) * 0.2).to(cuda).requires_grad_(True)
    tgt = torch.randint(0, K, (B, n), generator=g).to(cuda)
    keep = (torch.rand(B, n, generator=g) >= 0.36).to(cuda)
    tgt2 = torch.randint(0, K, (B, n), generator=g).to(cuda)
    keep2 = (torch.rand(B, n, generator=g) >= 0.7).to(cuda)
    assert int((~keep).sum()) != int((~keep2).sum())
    one = torch.ones((), device=cuda)

    def seg():
        loss = tied_logits_ce(h, W, bias, K, tgt, keep, one)
        return (loss.detach(),) + torch.autograd.grad(loss, (h, W, bias), one)

    sg = StepGraph([seg]).capture()
    tgt.copy_(tgt2)
    keep.copy_(keep2)
    got = [t.clone() for t in sg.replay()[0]]
    torch.cuda.synchronize()
    want = seg()
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
