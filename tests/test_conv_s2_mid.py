"""The stride-2 3x4 transposed gathers of the LF band's middle levels (64 -> 32 and 32 -> 16 reduction
to output channels, H = 3, widths 8-32): conv_s2m_t, the ConvTranspose forward and the replicate
conv's data gradient (folded onto dx inside the kernel).  tvq_conv_config bit 4096 turns it off.

B = 32 and B = 5 (an odd image count; one image per block).  Input width 17 gives the canvas form
50 columns per parity, a second pass over the column tiles.  Per case, for y, dx, dw, db: rel-L2
<= 1e-5 against torch float64 on the CPU and against the engine with bit 4096 set -- the bound
tests/test_conv_s2_ring.py and tests/test_ops_gpu.py use for these ops (fp32 reassociation only) --
and the plan lines show which kernels ran.  conv_s2m_t sums in the order of the split-K conv_tap
path it replaces, so wherever that path ran before the results are equal bit for bit (the
32 -> 16 shapes here, the 64 -> 32 ones at the step's B = 256).  Two eager runs are bitwise equal, a
captured graph replayed on two other inputs equals the eager results bitwise, and the eval-BN
entry point, whose launches must not have moved, equals its bit-4096 run bitwise.
"""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

OFF = 3 | 4096
# (transposed, Ci, Co, input width)
CASES = [(False, 16, 32, 32), (False, 32, 64, 16), (False, 32, 64, 17),
         (True, 64, 32, 8), (True, 32, 16, 16)]
REFUSED = [(False, 32, 64, 24), (True, 64, 32, 12)]  # output widths 24: not these kernels'


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


class _Engine:
    """Sets tvq_conv_config and restores it."""

    def __enter__(self):
        from timevqvae.hip._native import value
        self.value = value
        self.cfg = value("tvq_conv_config", -1)
        return self

    def set(self, cfg=3):
        self.value("tvq_conv_config", cfg)

    def __exit__(self, *exc):
        self.value("tvq_conv_config", self.cfg)


@functools.lru_cache(maxsize=None)
def _case(tr, Ci, Co, W, B):
    """Inputs and the torch float64 results of one case, computed once."""
    g = torch.Generator().manual_seed(1000 * Ci + 10 * Co + W + (7 if tr else 0) + 100000 * B)
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


def _traced(tr, dev):
    from timevqvae.hip._native import plan_trace
    with plan_trace() as trc:
        out = _fwd_bwd(tr, *dev)
        torch.cuda.synchronize()
    return out, trc


@pytest.mark.parametrize("B", [32, 5])
@pytest.mark.parametrize("tr,Ci,Co,W", CASES)
def test_mid_kernels_match_fp64_and_the_old_path(tr, Ci, Co, W, B, cuda):
    x, w, b, gy, ref = _case(tr, Ci, Co, W, B)
    dev = [t.to(cuda) for t in (x, w, b, gy)]
    with _Engine() as eng:
        eng.set(3)
        new, trc = _traced(tr, dev)
        again, _ = _traced(tr, dev)
        eng.set(OFF)
        old, trc_off = _traced(tr, dev)
    t_lines = trc.has("conv_s2m_t")
    assert len(t_lines) == 1, trc.lines
    if not tr:  # the replicate data gradient: folded in the kernel, no canvas launch
        assert " fold" in t_lines[0], trc.lines
        assert not [s for s in trc.lines if "hout5" in s and not s.startswith("conv_s2m_t")], trc.lines
    # the weight gradients stay where they were
    assert trc.has("conv_wgrad") == trc_off.has("conv_wgrad"), (trc.lines, trc_off.lines)
    assert not [s for s in trc_off.lines if "s2m" in s], trc_off.lines
    for n, a, a2, o, r in zip(("y", "dx", "dw", "db"), new, again, old, ref):
        print(f"{n}: vs float64 {rel(a, r):.3e}, vs bit 4096 {rel(a, o):.3e}")
        assert torch.equal(a, a2), f"{n}: two eager runs differ"
        assert rel(a, r) <= 1e-5, f"{n} against torch float64: {rel(a, r):.3e}"
        assert rel(a, o) <= 1e-5, f"{n} against the engine with bit 4096: {rel(a, o):.3e}"
        assert rel(o, r) <= 1e-5, f"{n}, bit 4096, against torch float64: {rel(o, r):.3e}"
        # at these batch sizes the 64-channel T gathers ran on conv_d32 (another order) before:
        # test_t_kernel_keeps_the_split_order_at_the_step_batch has them at B = 256
        if not (n == ("y" if tr else "dx") and max(Ci, Co) == 64):
            assert torch.equal(a, o), f"{n}: differs from the engine with bit 4096"


@pytest.mark.parametrize("tr,Ci,Co,W", [(False, 32, 64, 16), (True, 64, 32, 8)])
def test_t_kernel_keeps_the_split_order_at_the_step_batch(tr, Ci, Co, W, cuda):
    """B = 256, where the staged path is conv_tap with 6 splits: conv_s2m_t's chains are those
    splits, so y (ConvTranspose) and dx (replicate conv, fold included) are equal bit for bit."""
    x, w, b, gy, _ = _case(tr, Ci, Co, W, 256)
    dev = [t.to(cuda) for t in (x, w, b, gy)]
    with _Engine() as eng:
        eng.set(3)
        new, trc = _traced(tr, dev)
        eng.set(OFF)
        old, trc_off = _traced(tr, dev)
    assert trc.has("conv_s2m_t"), trc.lines
    assert trc_off.has("conv_tap splits6"), trc_off.lines
    k = 0 if tr else 1
    assert torch.equal(new[k], old[k])


@pytest.mark.parametrize("tr,Ci,Co,W", REFUSED)
def test_other_widths_keep_the_old_path(tr, Ci, Co, W, cuda):
    x, w, b, gy, ref = _case(tr, Ci, Co, W, 32)
    dev = [t.to(cuda) for t in (x, w, b, gy)]
    with _Engine() as eng:
        eng.set(3)
        new, trc = _traced(tr, dev)
        eng.set(OFF)
        old, trc_off = _traced(tr, dev)
    assert not [s for s in trc.lines if "s2m" in s], trc.lines
    assert trc.lines == trc_off.lines
    for n, a, o, r in zip(("y", "dx", "dw", "db"), new, old, ref):
        assert torch.equal(a, o), n
        assert rel(a, r) <= 1e-5, f"{n} against torch float64: {rel(a, r):.3e}"


@pytest.mark.parametrize("tr,Ci,Co,W", [(False, 32, 64, 16), (True, 64, 32, 8)])
def test_graph_replay_matches_eager(tr, Ci, Co, W, cuda):
    from timevqvae.hip.conv import conv2d, conv_transpose2d
    x0, w0, b0, gy0, _ = _case(tr, Ci, Co, W, 32)
    sets = []
    for k in range(3):
        g = torch.Generator().manual_seed(50 + k)
        sets.append([torch.randn(t.shape, generator=g).to(cuda) * s
                     for t, s in ((x0, 1.0), (w0, 0.2), (b0, 0.1), (gy0, 1.0))])
    with _Engine() as eng:
        eng.set(3)
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


def test_eval_bn_launch_has_not_moved(cuda):
    from timevqvae.hip._native import plan_trace
    from timevqvae.hip.conv import conv_transpose2d_bn_eval
    Ci, Co = 64, 32
    x, w, b, _, _ = _case(True, Ci, Co, 8, 32)
    x, w, b = (t.to(cuda) for t in (x, w, b))
    g = torch.Generator().manual_seed(Ci + Co)
    bn = nn.BatchNorm2d(Co).to(cuda).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(Co, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(Co, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(Co, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(Co, generator=g) + 0.3)
    a = (torch.rand(1, Co, 1, 1, generator=g) * 1.5 + 0.25).to(cuda)
    with _Engine() as eng, torch.no_grad():
        eng.set(3)
        with plan_trace() as trc:
            z = conv_transpose2d_bn_eval(x, w, b, bn, a)
            torch.cuda.synchronize()
        eng.set(OFF)
        with plan_trace() as trc_off:
            z_off = conv_transpose2d_bn_eval(x, w, b, bn, a)
            torch.cuda.synchronize()
    assert not [s for s in trc.lines if "s2m" in s], trc.lines
    assert trc.lines == trc_off.lines
    assert torch.equal(z, z_off)
