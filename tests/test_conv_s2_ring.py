"""The stride-2 small-channel convs (conv_s2f / conv_s2t / conv_wgrad_s2) with only the real
input rows staged and the stages walked through the two-buffer LDS ring (tvq_conv_s2_cap).

Shapes: B = 5 images of H = 3, so the stages never divide evenly over the blocks; widths at
the step's ragged and boundary cases; one channel pair per kernel instance (CS = 4 .. 16).
Checks, per case, for the forward, both data gradients (the fold form included), the weight
and bias gradients, the BatchNorm-statistics epilogue and the eval BN / Snake epilogue:

* ring against one-shot: the cap at the stage count (one stage per block), at 2 (every block
  wraps the ring and the last takes an uneven tail) and at 3 must agree bit for bit -- the
  arithmetic of a stage does not depend on which block runs it;
* row trimming against independent paths: the one-shot result against the engine without the
  stride-2 kernels (tvq_conv_config 3 | 512 | 1024) and against torch float64 on the CPU, at
  tests/test_ops_gpu.py's bound for these ops (rel-L2 <= 1e-5, fp32 reassociation only);
* the per-stage statistics against float64 sums of the stored output.  A partial is a sum of
  at most 3 x 64 fp32 values (or squares) accumulated in fp64 in a fixed order: against any
  other fp64 order it differs by at most 192 x 2^-53 < 1e-13 of the sum of magnitudes;
* a captured graph of one forward + backward replayed on two other inputs matches the eager
  results bit for bit: the ring keeps no state between launches.
"""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B = 5
PAIRS = [(12, 4), (4, 8), (8, 16), (16, 8), (4, 12), (12, 12)]
# Conv2d input widths: Wo = 128 (two segments), 64 (one), 32 (a half-empty segment), 16; 63:
# the canvas columns W, W + 1 straddle a segment, the data gradient is the unfolded T (Hout 5)
CONV_W = [257, 129, 65, 33, 63]
CONVT_W = [32, 256]  # -> 64 and 512
NO_S2 = 3 | 512 | 1024
ONE_SHOT = 1 << 30
CAPS = (ONE_SHOT, 2, 3)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


class _Engine:
    """Sets tvq_conv_s2_cap / tvq_conv_config and restores both."""

    def __enter__(self):
        from timevqvae.hip._native import value
        self.value = value
        self.cap = value("tvq_conv_s2_cap", -1)
        self.cfg = value("tvq_conv_config", -1)
        return self

    def set(self, cap=0, cfg=3):
        self.value("tvq_conv_s2_cap", cap)
        self.value("tvq_conv_config", cfg)

    def __exit__(self, *exc):
        self.value("tvq_conv_s2_cap", self.cap)
        self.value("tvq_conv_config", self.cfg)


@functools.lru_cache(maxsize=None)
def _case(tr, Ci, Co, W):
    """Inputs and the torch float64 results of one case, computed once."""
    g = torch.Generator().manual_seed(1000 * Ci + 10 * Co + W + (7 if tr else 0))
    x = torch.randn(B, Ci, 3, W, generator=g)
    w = torch.randn((Ci, Co, 3, 4) if tr else (Co, Ci, 3, 4), generator=g) * (Ci * 12) ** -0.5
    b = torch.randn(Co, generator=g) * 0.1
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    if tr:
        y = F.conv_transpose2d(xd, wd, bd, stride=(1, 2), padding=(1, 1))
    else:
        y = F.conv2d(F.pad(xd, (1, 1, 1, 1), mode="replicate"), wd, bd, stride=(1, 2))
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.double())
    return x, w, b, gy, (y.detach(), xd.grad, wd.grad, bd.grad)


def _fwd_bwd(tr, x, w, b, gy):
    from timevqvae.hip.conv import conv2d, conv_transpose2d
    x, w, b = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    y = conv_transpose2d(x, w, b) if tr else conv2d(x, w, b, stride_w=2, replicate=True)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), gy)
    return y.detach(), dx, dw, db


def _cases():
    for Ci, Co in PAIRS:
        for W in CONV_W:
            yield False, Ci, Co, W
        for W in CONVT_W:
            yield True, Ci, Co, W


@pytest.mark.parametrize("tr,Ci,Co,W", list(_cases()))
def test_ring_equals_one_shot_and_trimmed_rows_match(tr, Ci, Co, W, cuda):
    from timevqvae.hip._native import plan_trace
    x, w, b, gy, ref = _case(tr, Ci, Co, W)
    dev = [t.to(cuda) for t in (x, w, b, gy)]
    names = ("y", "dx", "dw", "db")
    with _Engine() as eng:
        runs = []
        for cap in CAPS:
            eng.set(cap=cap)
            with plan_trace() as trc:
                runs.append(_fwd_bwd(tr, *dev))
                torch.cuda.synchronize()
            assert trc.has("conv_s2t" if tr else "conv_s2f"), trc.lines
            assert trc.has("conv_s2f" if tr else "conv_s2t"), trc.lines
            assert trc.has("conv_wgrad_s2"), trc.lines
            if W != 63:
                assert tr or trc.has("conv_s2t_fold"), trc.lines
            if cap == 2:
                assert any(s.startswith("conv_s2") and "blocks=2 " in s for s in trc.lines), trc.lines
        eng.set(cfg=NO_S2)
        with plan_trace() as trc:
            other = _fwd_bwd(tr, *dev)
            torch.cuda.synchronize()
        assert not trc.has("conv_s2") and not trc.has("conv_wgrad_s2"), trc.lines
    for n, one, c2, c3 in zip(names, *runs):
        assert torch.equal(one, c2), f"{n}: cap 2 differs from one-shot"
        assert torch.equal(one, c3), f"{n}: cap 3 differs from one-shot"
    for n, one, o, r in zip(names, runs[0], other, ref):
        assert rel(one, o) <= 1e-5, f"{n} against the non-s2 path: {rel(one, o):.3e}"
        assert rel(one, r) <= 1e-5, f"{n} against torch float64: {rel(one, r):.3e}"


@pytest.mark.parametrize("tr,Ci,Co,W", [c for c in _cases() if c[3] != 63])
def test_stats_and_eval_epilogues(tr, Ci, Co, W, cuda):
    from timevqvae.hip.conv import (bnstats_blocks, conv2d_bn_eval, conv2d_bnstats,
                                    conv_transpose2d_bn_eval, conv_transpose2d_bnstats)
    from timevqvae.hip.norm import bn_snake
    x, w, b, _, ref = _case(tr, Ci, Co, W)
    x, w, b = (t.to(cuda) for t in (x, w, b))
    g = torch.Generator().manual_seed(Ci + Co)
    bn = nn.BatchNorm2d(Co).to(cuda).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(Co, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(Co, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(Co, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(Co, generator=g) + 0.3)
    a = (torch.rand(1, Co, 1, 1, generator=g) * 1.5 + 0.25).to(cuda)
    nblk = bnstats_blocks(x, w, 2, tr)
    Wo = ref[0].shape[3]
    segs = (Wo + 63) // 64
    assert nblk == B * segs
    with _Engine() as eng, torch.no_grad():
        stats, post = [], []
        for cap in CAPS:
            eng.set(cap=cap)
            y, part = (conv_transpose2d_bnstats(x, w, b) if tr
                       else conv2d_bnstats(x, w, b, stride_w=2, replicate=True))
            z = (conv_transpose2d_bn_eval(x, w, b, bn, a) if tr
                 else conv2d_bn_eval(x, w, b, bn, a, stride_w=2, replicate=True))
            torch.cuda.synchronize()
            stats.append((y, part))
            post.append(z)
        eng.set(cfg=NO_S2)
        from timevqvae.hip.conv import conv2d, conv_transpose2d
        h = conv_transpose2d(x, w, b) if tr else conv2d(x, w, b, stride_w=2, replicate=True)
        want = bn_snake(h, bn, a)
        torch.cuda.synchronize()
    for cap, (y, part), z in zip(CAPS[1:], stats[1:], post[1:]):
        assert torch.equal(stats[0][0], y), f"bnstats output, cap {cap}"
        assert torch.equal(stats[0][1], part), f"bnstats partials, cap {cap}"
        assert torch.equal(post[0], z), f"eval epilogue, cap {cap}"
    y, part = stats[0]
    assert rel(y, ref[0]) <= 1e-5
    assert rel(y, h) <= 1e-5
    # stage (image, segment) of channel n: float64 sums of the stored values
    yp = F.pad(y.double(), (0, segs * 64 - Wo)).view(B, Co, 3, segs, 64)
    s1 = yp.sum((2, 4)).permute(1, 0, 2).reshape(Co, nblk)
    s2 = (yp * yp).sum((2, 4)).permute(1, 0, 2).reshape(Co, nblk)
    m1 = yp.abs().sum((2, 4)).permute(1, 0, 2).reshape(Co, nblk)
    assert bool(((part[:, :, 0] - s1).abs() <= 1e-13 * m1).all())
    assert bool(((part[:, :, 1] - s2).abs() <= 1e-13 * s2).all())
    # tests/test_conv_bn_eval.py's bounds: 1e-6 of the two-launch path, 1e-5 of torch
    assert rel(post[0], want) < 1e-6, rel(post[0], want)
    yr = F.batch_norm(ref[0], bn.running_mean.double().cpu(), bn.running_var.double().cpu(),
                      bn.weight.double().cpu(), bn.bias.double().cpu(), False, 0.0, bn.eps)
    ad = a.double().cpu()
    assert rel(post[0], yr + (1.0 / ad) * torch.sin(ad * yr) ** 2) < 1e-5


@pytest.mark.parametrize("tr,Ci,Co,W", [(False, 12, 4, 257), (True, 12, 12, 256)])
def test_graph_replay_matches_eager(tr, Ci, Co, W, cuda):
    from timevqvae.hip.conv import conv2d, conv_transpose2d
    x0, w0, b0, gy0, _ = _case(tr, Ci, Co, W)
    sets = []
    for k in range(3):
        g = torch.Generator().manual_seed(50 + k)
        sets.append([torch.randn(t.shape, generator=g).to(cuda) * s
                     for t, s in ((x0, 1.0), (w0, 0.2), (b0, 0.1), (gy0, 1.0))])
    with _Engine() as eng:
        eng.set(cap=2)
        eager = [_fwd_bwd(tr, *s) for s in sets]
        torch.cuda.synchronize()
        x, w, b = (t.clone().requires_grad_(True) for t in sets[0][:3])
        gy = sets[0][3].clone()

        def step():
            y = conv_transpose2d(x, w, b) if tr else conv2d(x, w, b, stride_w=2, replicate=True)
            return (y.detach(),) + torch.autograd.grad(y, (x, w, b), gy)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step()
        for k in (1, 2):
            with torch.no_grad():
                for dst, src in zip((x, w, b, gy), sets[k]):
                    dst.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            for n, got, want in zip(("y", "dx", "dw", "db"), outs, eager[k]):
                assert torch.equal(got, want), f"replay {k}: {n}"
