"""The LF band's middle stride-2 T gathers at the step's B = 256 shapes, one launch at a time: the
two ConvTranspose forwards and the two replicate conv data gradients, conv_s2m_t against the path
it replaces (tvq_conv_config bit 4096).  Each timing is a captured graph of 20 launches, replayed 7
times, best replay / 20.
usage: python tools/ab/s2_mid_inst.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "t-vq-vae-trajgen_amd"))

from timevqvae.hip import _native  # noqa: E402
from timevqvae.hip import conv as hconv  # noqa: E402
from timevqvae.hip.conv import conv2d, conv_transpose2d  # noqa: E402

B, REP = 256, 20
SHAPES = [(False, 16, 32, 32), (False, 32, 64, 16), (True, 64, 32, 8), (True, 32, 16, 16)]
dev = torch.device("cuda:0")


def timed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REP):
            fn()
    best = 1e9
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / REP)
    return best


print("us per launch: bit 4096 (old path) / new", flush=True)
for tr, Ci, Co, W in SHAPES:
    torch.manual_seed(0)
    x = torch.randn(B, Ci, 3, W, device=dev)
    w = torch.randn((Ci, Co, 3, 4) if tr else (Co, Ci, 3, 4), device=dev) * 0.1
    b = torch.zeros(Co, device=dev)
    with torch.no_grad():
        y = conv_transpose2d(x, w, b) if tr else conv2d(x, w, b, stride_w=2, replicate=True)
    gy = torch.randn_like(y)
    Wo = gy.shape[3]
    dx = torch.empty_like(x)
    sp = _native.stream_ptr
    if tr:
        t = lambda: conv_transpose2d(x, w, b)  # noqa: E731
    else:
        ws = hconv._conv_ws(hconv.OP_DGRAD, dev, B, Ci, 3, W, Co, 3, 4, 2, 1, required=True)
        t = lambda: _native.call("tvq_conv2d_dgrad", gy.data_ptr(), B, Co, 3, Wo, w.data_ptr(), Ci, 3,  # noqa: E731
                                 4, 2, 1, dx.data_ptr(), W, ws.data_ptr(), sp())
    row = []
    for cfg in (3 | 4096, 3):
        _native.value("tvq_conv_config", cfg)
        with torch.no_grad():
            row.append(timed(t))
    name = f"{'convT' if tr else 'conv '} {Ci:2d}->{Co:2d} W{W:3d}"
    print(f"{name} {'fwd  ' if tr else 'dgrad'} {row[0]:7.2f} / {row[1]:7.2f}", flush=True)
