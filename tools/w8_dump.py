"""Every result of the fused W = 8 ResBlocks (csrc/tvq_resblock_w8*.hip) as .npy files, for a
byte-for-byte comparison of two builds: the identity block (64, 64), the fused pair of two of
them, and the projection blocks (64, 128) and (128, 64) on seeded (5, C, 3, 8) inputs with
dropout 0.3.  Per case: the training forward + backward with the gradients returned
(accumulate = 0) and accumulated into preset .grad buffers (accumulate = 1) -- y, every
gradient, the BN buffers and the tensors saved for the backward (h | s1 | s2, `save`) -- and
the eval forward outside and inside a pack-cache scope.  Uses timevqvae.hip.resblock and the
models only.

usage: python tools/w8_dump.py OUT_DIR      then: diff -r OUT_DIR_A OUT_DIR_B"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "t-vq-vae-trajgen_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, DROP = 5, 0.3
CASES = [("id64", 64, 64, 1), ("pair64", 64, 64, 2), ("proj64_128", 64, 128, 1),
         ("proj128_64", 128, 64, 1)]


def blocks(Ci, Co, n):
    from timevqvae.hip import rng
    from timevqvae.models.vq_vae import ResBlock
    rng.manual_seed(1234)
    ms = []
    for i in range(n):
        torch.manual_seed(10 + i)
        m = ResBlock(Ci, Co, False, dropout=DROP)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn_like(p) * (0.3 if p.dim() > 1 else 0.5))
            m.convs[0].a.uniform_(0.3, 0.8)
            m.convs[3].a.uniform_(0.3, 0.8)
            m.convs[2].running_mean.normal_()
            m.convs[2].running_var.uniform_(0.5, 2.0)
        ms.append(m.cuda())
    return ms


def main(out):
    from timevqvae.hip import resblock, rng
    from timevqvae.hip.conv import PackCache
    from timevqvae.models.vq_vae import run_layers
    os.makedirs(out, exist_ok=True)

    def put(name, t):
        np.save(os.path.join(out, name + ".npy"), t.detach().cpu().numpy())

    for tag, Ci, Co, n in CASES:
        torch.manual_seed(7)
        x = torch.randn(B, Ci, 3, 8, device="cuda")
        assert resblock.supported(x, Ci, Co) or resblock.proj_supported(x, Ci, Co)
        assert n == 1 or resblock.pair_supported(x)
        for acc in (0, 1):
            ms = blocks(Ci, Co, n)
            for m in ms:
                m.train(True)
                for p in m.parameters():
                    if acc:  # the backward kernels add into .grad (hip._native.grad_sink)
                        p._tvq_flat = True
                        p.grad = torch.sin(torch.arange(p.numel(), device="cuda",
                                                        dtype=torch.float32)).view_as(p)
            rng.restart_calls()
            xx = x.clone().requires_grad_(True)
            y = run_layers(ms, xx, lambda layer, v: layer(v))
            for i, t in enumerate(y.grad_fn.saved_tensors):
                put(f"{tag}_acc{acc}_saved{i}", t)
            gy = torch.cos(torch.arange(y.numel(), device="cuda", dtype=torch.float32)).view_as(y)
            y.backward(gy)
            torch.cuda.synchronize()
            put(f"{tag}_acc{acc}_y", y)
            put(f"{tag}_acc{acc}_dx", xx.grad)
            for i, m in enumerate(ms):
                for k, p in m.named_parameters():
                    put(f"{tag}_acc{acc}_b{i}_grad_{k}", p.grad)
                for k, b in m.named_buffers():
                    put(f"{tag}_acc{acc}_b{i}_buf_{k}", b)
        ms = blocks(Ci, Co, n)
        for m in ms:
            m.eval()
        with torch.no_grad():
            v = x
            for m in ms:
                v = m(v)
            put(f"{tag}_eval_raw", v)
            with PackCache(x.device).scope():
                v = x
                for m in ms:
                    v = m(v)
                put(f"{tag}_eval_packed", v)
        torch.cuda.synchronize()
    print(f"w8_dump: {len(os.listdir(out))} files in {out}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
