"""Stride-2 small-channel convs at the step's B = 256 shapes: time of the forward launch, of the
data-gradient launch and of the eval (BN + Snake epilogue) forward per instance, for a list of
tvq_conv_s2_cap values (0 = the production choice, 1073741824 = one-shot).  Each timing is a
captured graph of 20 launches, replayed 7 times, best replay / 20.  A tree whose library has no
tvq_conv_s2_cap is timed once.  --root TREE times another checkout's build.
usage: python tools/ab/s2_ring_cap.py [--root TREE] [--caps 0,1073741824,256,512,1024]"""
import argparse
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--caps", default="0,1073741824,256,512,768,1024,2048")
args = ap.parse_args()
sys.path.insert(0, os.path.join(args.root, "t-vq-vae-trajgen_amd"))

from timevqvae.hip import _native  # noqa: E402
from timevqvae.hip import conv as hconv  # noqa: E402
from timevqvae.hip.conv import (conv2d, conv2d_bn_eval, conv_transpose2d,  # noqa: E402
                                conv_transpose2d_bn_eval)

B, REP = 256, 20
# (transposed, Ci, Co, input width): EncBlocks, DecBlocks and the decoders' tails of both bands
SHAPES = [(False, 12, 4, 513), (False, 12, 4, 257), (False, 4, 8, 257), (False, 4, 8, 129),
          (False, 8, 16, 129), (False, 8, 16, 65), (True, 16, 8, 32), (True, 8, 4, 64),
          (True, 16, 8, 64), (True, 8, 4, 128), (True, 4, 12, 128), (True, 12, 12, 256),
          (True, 4, 12, 64), (True, 12, 12, 128)]
dev = torch.device("cuda:0")
has_cap = hasattr(_native.lib(), "tvq_conv_s2_cap")
caps = [int(c) for c in args.caps.split(",")] if has_cap else [None]


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


print("us per launch; caps:", caps, flush=True)
for tr, Ci, Co, W in SHAPES:
    torch.manual_seed(0)
    x = torch.randn(B, Ci, 3, W, device=dev)
    w = torch.randn((Ci, Co, 3, 4) if tr else (Co, Ci, 3, 4), device=dev) * 0.1
    b = torch.zeros(Co, device=dev)
    f = (lambda: conv_transpose2d(x, w, b)) if tr else (lambda: conv2d(x, w, b, stride_w=2, replicate=True))
    with torch.no_grad():
        gy = torch.randn_like(f())
    Wo = gy.shape[3]
    # the data gradient through its C entry point, on the capturing stream (a backward node of
    # a forward that ran outside the capture would launch on the forward's stream)
    dx = torch.empty_like(x)
    ws = hconv._conv_ws(hconv.OP_T_DGRAD if tr else hconv.OP_DGRAD, dev, B, Ci, 3, W, Co, 3, 4, 2,
                        0 if tr else 1, required=True)
    if tr:
        d = lambda: _native.call("tvq_convT2d_dgrad", gy.data_ptr(), B, Co, 3, Wo, w.data_ptr(), Ci, 3,  # noqa: E731
                                 4, 2, dx.data_ptr(), W, ws.data_ptr(), _native.stream_ptr())
    else:
        d = lambda: _native.call("tvq_conv2d_dgrad", gy.data_ptr(), B, Co, 3, Wo, w.data_ptr(), Ci, 3,  # noqa: E731
                                 4, 2, 1, dx.data_ptr(), W, ws.data_ptr(), _native.stream_ptr())
    bn = torch.nn.BatchNorm2d(Co).to(dev).eval()
    a = torch.full((1, Co, 1, 1), 0.5, device=dev)
    e = ((lambda: conv_transpose2d_bn_eval(x, w, b, bn, a)) if tr
         else (lambda: conv2d_bn_eval(x, w, b, bn, a, stride_w=2, replicate=True)))
    row_f, row_d, row_e = [], [], []
    for cap in caps:
        if cap is not None:
            _native.value("tvq_conv_s2_cap", cap)
        with torch.no_grad():
            row_f.append(timed(f))
            row_d.append(timed(d))
            row_e.append(timed(e))
    if has_cap:
        _native.value("tvq_conv_s2_cap", 0)
    name = f"{'convT' if tr else 'conv '} {Ci:2d}->{Co:2d} W{W:3d}"
    print(name, "fwd  ", " ".join(f"{t:7.2f}" for t in row_f), flush=True)
    print(name, "dgrad", " ".join(f"{t:7.2f}" for t in row_d), flush=True)
    print(name, "eval ", " ".join(f"{t:7.2f}" for t in row_e), flush=True)
