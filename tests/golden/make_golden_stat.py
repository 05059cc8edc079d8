"""Generate the G13 golden (TSGBench statistics MDD / ACD / SD / KD) from the REFERENCE
timevqvae/evaluation/stat_metrics.py (:5-60).

Runs only where the reference checkout exists (the build container); the reference file is
loaded by path exactly as make_golden.py does.  Only the .npz output is committed:

    tests/golden/g13_stat.npz
      a_real (5,3,65), a_gen (7,3,65)   float64 random walks (cumsum * 0.1); a_out = the
                                        reference's (mdd, acd, sd, kd)
      b_real (3,1,2), b_gen (4,1,2)     float64; b_out
      c_real, c_gen                     the case-a inputs cast to float32; c_out32 = the
                                        reference on the float32 arrays, c_out64 = the
                                        reference on those same values as float64

    python tests/golden/make_golden_stat.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, _load  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
NAMES = ("marginal_distribution_difference", "auto_correlation_difference",
         "skewness_difference", "kurtosis_difference")


def walks(rng, shape, offset):
    return offset + np.cumsum(rng.standard_normal(shape), axis=-1) * 0.1


def run(ref, real, gen):
    return np.array([float(getattr(ref, n)(real, gen)) for n in NAMES], dtype=np.float64)


def main():
    ref = _load("ref_stat_metrics", f"{REF}/evaluation/stat_metrics.py")
    rng = np.random.default_rng(13)
    d = {}
    d["a_real"], d["a_gen"] = walks(rng, (5, 3, 65), 0.0), walks(rng, (7, 3, 65), 0.2)
    d["a_out"] = run(ref, d["a_real"], d["a_gen"])
    d["b_real"], d["b_gen"] = walks(rng, (3, 1, 2), 0.0), walks(rng, (4, 1, 2), 0.2)
    d["b_out"] = run(ref, d["b_real"], d["b_gen"])
    d["c_real"], d["c_gen"] = d["a_real"].astype(np.float32), d["a_gen"].astype(np.float32)
    d["c_out32"] = run(ref, d["c_real"], d["c_gen"])
    d["c_out64"] = run(ref, d["c_real"].astype(np.float64), d["c_gen"].astype(np.float64))
    for k in ("a_out", "b_out", "c_out32", "c_out64"):
        assert np.isfinite(d[k]).all(), (k, d[k])
        print(k, " ".join(f"{v:.17g}" for v in d[k]))
    print("float32 / float64 relative gap", np.abs(d["c_out32"] - d["c_out64"]) / np.abs(d["c_out64"]))
    path = os.path.join(OUT, "g13_stat.npz")
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(f"wrote g13_stat.npz: {size} bytes")


if __name__ == "__main__":
    main()
