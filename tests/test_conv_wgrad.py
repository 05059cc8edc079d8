"""tvq_conv2d_wgrad / tvq_convT2d_wgrad called directly, one small shape per kernel family, in
a workspace of exactly tvq_conv_workspace(4 | 5, ...) floats cut out of a larger tensor with
1024 sentinel floats on either side: a family whose launch and whose workspace size disagreed
about the split count would write into a guard.  Each case asserts by the plan trace that it
took the family it is listed under."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import WGRAD_VARIANTS, close

pytestmark = pytest.mark.gpu

GUARD = 1024          # sentinel floats in front of and behind the workspace (a multiple of 64)
SENTINEL = 0x7FC0BEEF  # a NaN's bits: compared as int32

# name: (family's plan line, transposed, (B, Ci, Co, H, W), (KH, KW), SW, replicate).
# The transpose cases' G is x: conv_wgrad_s2 takes them while both channel counts are <= 16, so
# the halo and split cases have 32 and 20 input channels; the split case's width is no
# multiple of 4, which the halo kernel needs.
CASES = {
    "t32": ("conv_wgrad_t32", False, (2, 64, 64, 1, 32), (1, 3), 1, False),
    "halo": ("conv_wgrad_halo", False, (3, 6, 8, 1, 256), (1, 7), 1, False),
    "split": ("conv_wgrad split=", False, (2, 6, 8, 1, 301), (1, 7), 1, False),
    "s2": ("conv_wgrad_s2", False, (2, 16, 16, 3, 128), (3, 4), 2, True),
    "w8": ("conv_wgrad_w8", False, (16, 8, 32, 3, 8), (3, 3), 1, False),
    "T_s2": ("conv_wgrad_s2", True, (2, 16, 16, 3, 40), (3, 4), 2, False),
    "T_halo": ("conv_wgrad_halo", True, (2, 32, 4, 3, 64), (3, 4), 2, False),
    "T_split": ("conv_wgrad split=", True, (3, 20, 7, 3, 37), (3, 4), 2, False),
}
# (case, db given): tvq_convT2d_wgrad has no db
RUNS = [(n, b) for n, c in CASES.items() for b in ((False,) if c[1] else (False, True))]


@functools.lru_cache(maxsize=None)
def reference(name):
    """Seeded x, upstream gradient g and initial dw0 / db0, with the CPU float32 gradients."""
    _, transposed, (B, Ci, Co, H, W), (KH, KW), SW, rep = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(B, Ci, H, W, generator=gen)
    w = torch.randn((Ci, Co, KH, KW) if transposed else (Co, Ci, KH, KW), generator=gen,
                    requires_grad=True)
    b = torch.randn(Co, generator=gen, requires_grad=True)
    pad = (KH // 2, (KW - 1) // 2)
    if transposed:
        y = F.conv_transpose2d(x, w, b, stride=(1, SW), padding=pad)
    elif rep:
        y = F.conv2d(F.pad(x, (pad[1], pad[1], pad[0], pad[0]), mode="replicate"), w, b,
                     stride=(1, SW))
    else:
        y = F.conv2d(x, w, b, stride=(1, SW), padding=pad)
    g = torch.randn(y.shape, generator=gen)
    y.backward(g)
    dw0 = torch.randn(w.shape, generator=gen)
    db0 = torch.randn(Co, generator=gen)
    return x, g, dw0, db0, w.grad, b.grad


def run_wgrad(name, with_db, accumulate, deferred, dev):
    """One direct call in a guarded workspace -> (dw, db or None, guards untouched, plan lines)."""
    from timevqvae.hip._native import call, plan_trace, ptr, stream_ptr, value
    from timevqvae.hip.conv import wgrad_deferred
    _, transposed, (B, Ci, Co, H, W), (KH, KW), SW, rep = CASES[name]
    x, g, dw0, db0, _, _ = reference(name)
    xd, gd = x.to(dev), g.to(dev)
    dw = dw0.to(dev)
    db = db0.to(dev) if with_db else None
    n = value("tvq_conv_workspace", 5 if transposed else 4, B, Ci, H, W, Co, KH, KW, SW, int(rep))
    buf = torch.empty(GUARD + n + GUARD, device=dev, dtype=torch.float32)
    buf.view(torch.int32).fill_(SENTINEL)
    ws = buf[GUARD:GUARD + n]
    assert ws.data_ptr() % 256 == 0
    Wo = g.shape[3]
    with plan_trace() as tr, (wgrad_deferred() if deferred else contextlib.nullcontext()):
        if transposed:
            call("tvq_convT2d_wgrad", ptr(xd), B, Ci, H, W, ptr(gd), Co, Wo, KH, KW, SW, ptr(dw),
                 accumulate, ptr(ws), stream_ptr())
        else:
            call("tvq_conv2d_wgrad", ptr(xd), B, Ci, H, W, ptr(gd), Co, Wo, KH, KW, SW, int(rep),
                 ptr(dw), ptr(db), accumulate, ptr(ws), stream_ptr())
    torch.cuda.synchronize()
    guards = torch.cat([buf[:GUARD], buf[GUARD + n:]]).view(torch.int32)
    return dw.cpu(), None if db is None else db.cpu(), bool((guards == SENTINEL).all()), tr.lines


@pytest.mark.parametrize("deferred", [False, True], ids=["now", "deferred"])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("name,with_db", RUNS)
def test_wgrad_in_exact_workspace(name, with_db, accumulate, deferred, cuda):
    """dw / db against the CPU F.conv2d / F.conv_transpose2d gradients (test_conv2d's
    tolerance), the guards around the exactly sized workspace untouched, the family pinned."""
    family = CASES[name][0]
    _, _, dw0, db0, dw_ref, db_ref = reference(name)
    dw, db, guards_ok, lines = run_wgrad(name, with_db, accumulate, deferred, cuda)
    took = [v for v in WGRAD_VARIANTS if any(s.startswith(v) for s in lines)]
    assert took == [family], (took, lines)
    assert guards_ok, "the kernel or its split sum wrote outside tvq_conv_workspace's floats"
    close(dw - dw0 if accumulate else dw, dw_ref, what="dw")
    if with_db:
        close(db - db0 if accumulate else db, db_ref, what="db")


def test_cases_cover_every_family():
    assert {c[0] for c in CASES.values()} == set(WGRAD_VARIANTS)
    assert {c[0] for c in CASES.values() if c[1]} == {"conv_wgrad_s2", "conv_wgrad_halo",
                                                     "conv_wgrad split="}
