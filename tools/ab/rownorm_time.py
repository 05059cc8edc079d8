"""The RMSNorm / LayerNorm C entry points alone at the rows the joint step launches at B = 256
-- (6400, 128) in the LF prior and (24832, 32) in the HF prior, and the LayerNorms at (6144, 128)
and (24576, 128) -- forward and backward of both operators, the RMSNorm backward with and
without the residual gradient; and the forward at the sampler's (99328, 32) and (99328, 128)
(1024 trajectories x 97 HF tokens).  Each timing is a captured graph of
20 launches, replayed 7 times, best replay / 20.  --root TREE times another checkout's build.
usage: python tools/ab/rownorm_time.py [--root TREE]"""
import argparse
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
args = ap.parse_args()
sys.path.insert(0, os.path.join(args.root, "t-vq-vae-trajgen_amd"))

from timevqvae.hip import _native  # noqa: E402

REP = 20
SHAPES = [(6400, 128, True), (24832, 32, True), (6144, 128, True), (24576, 128, True),
          (99328, 32, False), (99328, 128, False)]  # M, D, backward too
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


print("us per call", flush=True)
for M, D, bwd in SHAPES:
    torch.manual_seed(0)
    x = torch.randn(M, D, device=dev) * 3 + 0.5
    dy, dres = torch.randn(M, D, device=dev), torch.randn(M, D, device=dev)
    g, b = torch.rand(D, device=dev) + 0.5, torch.randn(D, device=dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    s0, s1 = torch.empty(M, device=dev), torch.empty(M, device=dev)
    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    ws = torch.empty(_native.value("tvq_norm_bwd_workspace", M, D), device=dev)
    p, st = (lambda t: t.data_ptr()), _native.stream_ptr
    runs = [("rmsnorm_fwd", lambda: _native.call("tvq_rmsnorm_fwd", p(x), M, D, p(g), D ** 0.5, p(y),
                                                 p(s0), st())),
            ("layernorm_fwd", lambda: _native.call("tvq_layernorm_fwd", p(x), M, D, p(g), p(b), 1e-5,
                                                   p(y), p(s0), p(s1), st()))]
    if bwd:
        runs += [("rmsnorm_bwd", lambda: _native.call("tvq_rmsnorm_bwd", p(dy), p(x), M, D, p(g), D ** 0.5,
                                                      p(s0), None, p(dx), p(dg), 0, p(ws), st())),
                 ("rmsnorm_bwd+dres", lambda: _native.call("tvq_rmsnorm_bwd", p(dy), p(x), M, D, p(g),
                                                           D ** 0.5, p(s0), p(dres), p(dx), p(dg), 0,
                                                           p(ws), st())),
                 ("layernorm_bwd", lambda: _native.call("tvq_layernorm_bwd", p(dy), p(x), M, D, p(g),
                                                        p(s0), p(s1), p(dx), p(dg), p(db), 0, p(ws),
                                                        st()))]
    for name, fn in runs:  # each backward reads the statistics its operator's forward left
        if name.startswith("rmsnorm_bwd"):
            runs[0][1]()
        elif name == "layernorm_bwd":
            runs[1][1]()
        print(f"({M:5d}, {D:3d}) {name:17s} {timed(fn):7.2f}", flush=True)
