"""What the conv weight-gradient entry points size and compute, as files, for a byte-for-byte
comparison of two builds.

  sizes.txt   tvq_conv_workspace(4 | 5, ...) over a grid: the model's conv shapes (the LF / HF
              bands' and the HF prior's Upscale, tools/conv_shapes_bench.py) and the
              FidelityEnhancer's (FE_CONVS of tests/test_ops_gpu.py), each at B in
              {1, 2, 16, 37, 256} and, FE, at its own B; the cases of tests/test_conv_wgrad.py.
              Needs the loaded library only, no device.
  *.npy       with a device: dw (and db) of every run of tests/test_conv_wgrad.py -- each case
              with db given and absent, accumulate 0 and 1, at once and inside wgrad_deferred()
  plans.txt   those runs' plan lines (without the flush's, which print a stream's address)

Uses the package's public functions only, so --root TREE dumps another checkout's build.

usage: python tools/wgrad_dump.py [--root TREE] OUT_DIR    then: diff -r OUT_DIR_A OUT_DIR_B"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser(usage=__doc__)
ap.add_argument("--root", default=HERE)
ap.add_argument("out")
args = ap.parse_args()
sys.path[:0] = [os.path.join(args.root, "t-vq-vae-trajgen_amd"), os.path.join(HERE, "tests"),
                os.path.join(HERE, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from timevqvae.hip._native import LIB_PATH, value  # noqa: E402  (--root's, before the imports below)
from conv_shapes_bench import SHAPES  # noqa: E402
from test_conv_wgrad import CASES, RUNS, run_wgrad  # noqa: E402
from test_ops_gpu import FE_CONVS  # noqa: E402

BATCHES = (1, 2, 16, 37, 256)


def grid():
    """(op, B, Ci, H, Wi, Co, KH, KW, SW, replicate) in a fixed order, without repeats."""
    rows = []
    for _, Ci, Co, H, W, KH, KW, SW, rep, transposed in SHAPES:
        rows += [(5 if transposed else 4, B, Ci, H, W, Co, KH, KW, SW, rep) for B in BATCHES]
    for B0, Ci, Co, L, K, S, rep, _ in FE_CONVS:
        rows += [(4, B, Ci, 1, L, Co, 1, K, S, int(rep)) for B in (B0,) + BATCHES]
    for _, transposed, (B, Ci, Co, H, W), (KH, KW), SW, rep in CASES.values():
        rows.append((5 if transposed else 4, B, Ci, H, W, Co, KH, KW, SW, int(rep)))
    return list(dict.fromkeys(rows))


def main(out):
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "sizes.txt"), "w") as f:
        for row in grid():
            f.write(" ".join(map(str, row)) + f" -> {value('tvq_conv_workspace', *row)}\n")
    if not torch.cuda.is_available():
        print(f"wgrad_dump: sizes only (no device) in {out}, from {LIB_PATH}")
        return
    dev = torch.device("cuda:0")
    with open(os.path.join(out, "plans.txt"), "w") as f:
        for name, with_db in RUNS:
            for accumulate in (0, 1):
                for deferred in (False, True):
                    tag = f"{name}_db{int(with_db)}_acc{accumulate}_{'deferred' if deferred else 'now'}"
                    dw, db, guards_ok, lines = run_wgrad(name, with_db, accumulate, deferred, dev)
                    np.save(os.path.join(out, tag + "_dw.npy"), dw.numpy())
                    if db is not None:
                        np.save(os.path.join(out, tag + "_db.npy"), db.numpy())
                    kept = [s for s in lines if not s.startswith("wgrad_flush")]
                    f.write(f"{tag} guards_ok={guards_ok}: " + " | ".join(kept) + "\n")
    print(f"wgrad_dump: {len(os.listdir(out))} files in {out}, from {LIB_PATH}")


if __name__ == "__main__":
    main(args.out)
