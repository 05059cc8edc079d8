"""Every result of the RMSNorm / LayerNorm row-norm kernels (csrc/tvq_rownorm.hip) as .npy
files, for a byte-for-byte comparison of two builds.  Cases: RMSNorm without and with the
residual gradient (rmsnorm, rmsnorm_res with both outputs used), LayerNorm with (gamma, beta),
gamma only and neither, on seeded inputs at every (D, M) of tests/test_rownorm.py -- each
arm of the forward and backward dispatch and of the row bookkeeping -- and at the training
step's own shapes (6400, 128) and (24832, 32).  Per case, with the parameter gradients
returned (accumulate = 0) and added into preset .grad buffers (accumulate = 1): y, the saved
statistics (inv_norm, or mean and rstd), dx and every parameter gradient.  Uses
timevqvae.hip.xf's public functions only, so --root TREE dumps another checkout's build.

usage: python tools/rownorm_dump.py [--root TREE] OUT_DIR    then: diff -r OUT_DIR_A OUT_DIR_B"""
import argparse
import os
import sys

ap = argparse.ArgumentParser(usage=__doc__)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("out")
args = ap.parse_args()
sys.path.insert(0, os.path.join(args.root, "t-vq-vae-trajgen_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from timevqvae.hip.xf import layer_norm, rmsnorm, rmsnorm_res  # noqa: E402

DS = [8, 32, 48, 64, 100, 128, 200, 256, 320]
MS = [1, 5, 1031, 2300]
SHAPES = [(D, M) for D in DS for M in MS] + [(128, 6400), (32, 24832)]
CASES = ["rms", "rms_res", "ln_gb", "ln_g", "ln"]


def main(out):
    os.makedirs(out, exist_ok=True)

    def put(name, t):
        np.save(os.path.join(out, name + ".npy"), t.detach().cpu().numpy())

    for D, M in SHAPES:
        gen = torch.Generator().manual_seed(1000 * D + M)
        x = torch.randn(M, D, generator=gen) * 3 + 0.5
        gy = torch.randn(M, D, generator=gen).cuda()
        gr = torch.randn(M, D, generator=gen).cuda()
        g = torch.rand(D, generator=gen) + 0.5
        b = torch.randn(D, generator=gen)
        for case in CASES:
            for acc in (0, 1):
                xd = x.cuda().requires_grad_(True)
                p = {}
                if case != "ln":
                    p["g"] = g.cuda().requires_grad_(True)
                if case == "ln_gb":
                    p["b"] = b.cuda().requires_grad_(True)
                for v in p.values():
                    if acc:  # the backward kernels add into .grad (hip._native.grad_sink)
                        v._tvq_flat = True
                        v.grad = torch.sin(torch.arange(D, device="cuda", dtype=torch.float32))
                if case == "rms":
                    outs, gouts = [rmsnorm(xd, p["g"])], [gy]
                elif case == "rms_res":
                    outs, gouts = list(rmsnorm_res(xd, p["g"])), [gy, gr]
                else:
                    outs, gouts = [layer_norm(xd, p.get("g"), p.get("b"), 1e-5)], [gy]
                tag = f"{case}_D{D}_M{M}_acc{acc}"
                stats = [t for t in outs[0].grad_fn.saved_tensors if t is not None and t.shape == (M,)]
                assert len(stats) == (1 if case.startswith("rms") else 2), tag
                for i, t in enumerate(stats):
                    put(f"{tag}_stat{i}", t)
                torch.autograd.backward(outs, gouts)
                torch.cuda.synchronize()
                put(f"{tag}_y", outs[0])
                put(f"{tag}_dx", xd.grad)
                for k, v in p.items():
                    put(f"{tag}_d{k}", v.grad)
    print(f"rownorm_dump: {len(os.listdir(out))} files in {out}")


if __name__ == "__main__":
    main(args.out)
