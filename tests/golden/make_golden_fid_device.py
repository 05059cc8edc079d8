"""Generate the G16 golden (FID end to end on the device) from the REFERENCE
timevqvae/evaluation/eval_utils.py calculate_fid (:56-81).

Runs only where the reference checkout exists (the build container); the reference file is
loaded by path as make_golden.gen_fid does, its FCNBaseline import stubbed (calculate_fid
never uses it).  Only the .npz output is committed:

    tests/golden/g16_fid_device.npz
      names                   the case names, "few_*" then "many_*"
      <case>_z1, <case>_z2    the feature sets (float64; float32 for few_f32)
      <case>_ref              the reference's calculate_fid(z1, z2)
      <case>_lap              the same scalar with tr sqrtm(sigma1 sigma2) stated as the sum of
                              numpy.linalg.svd's singular values of A1 A2^T, A_i = (z_i - mu_i)
                              / sqrt(N_i - 1) in float64 (fid_jacobi_model.fid_lapack)
      <case>_tr               tr sigma1 + tr sigma2, the scale of every tolerance
      <case>_ref_gap          |ref - lap|

Rows are L2-normalised Gaussian features from default_rng(16); the second set is scaled by
1.3 and shifted by 0.2.  Cases as (N1, N2, D):
  few  (min(N1, N2) <= D, singular covariances): (33, 47, 64); (60, 50, 100) with two constant
       feature columns, as ROCKET ppv columns can be; (48, 70, 48), N = D; (40, 40, 96),
       identical sets; (2, 2, 3); (90, 80, 128) in float32.
  many (min(N1, N2) > D): (49, 70, 48), N = D + 1; (300, 250, 40); (200, 150, 48) with feature
       j scaled by exp(-0.2 j); (120, 90, 32) with two constant columns; (150, 150, 24),
       identical sets.

Asserted here: ref_gap <= 1e-7 tr on the few cases (the reference's sqrtm of a singular
non-symmetric product; measured 3.3e-9 .. 1.3e-8 tr, except 2.6e-15 tr on (48, 70, 48), where
sigma2 is regular) and <= 1e-12 tr on the many cases (measured <= 4.4e-16 tr), and that the
numpy statement of the device algorithm (fid_jacobi_model.fid_jacobi) converges within 20
sweeps on every case (measured 3 .. 12) and lands within 1e-12 tr of lap (measured <=
8.3e-16 tr).  No case had to be redrawn.

    python tests/golden/make_golden_fid_device.py
"""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fid_jacobi_model import fid_jacobi, fid_lapack  # noqa: E402
from make_golden import REF, _load  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def load_eval_utils():
    pkg = types.ModuleType("timevqvae")
    pkg.__path__ = []
    sys.modules["timevqvae"] = pkg
    models = types.ModuleType("timevqvae.models")
    models.FCNBaseline = object
    sys.modules["timevqvae.models"] = models
    return _load("ref_eval_utils", f"{REF}/evaluation/eval_utils.py")


def feats(rng, n, d):
    z = rng.standard_normal((n, d))
    return z / np.linalg.norm(z, axis=1, keepdims=True)


def pair(rng, n1, n2, d):
    return feats(rng, n1, d), 1.3 * feats(rng, n2, d) + 0.2


def const_cols(z1, z2):
    for z in (z1, z2):
        z[:, 3] = 1.0
        z[:, z.shape[1] - 2] = 0.0
    return z1, z2


def cases(rng):
    c = {}
    c["few_a"] = pair(rng, 33, 47, 64)
    c["few_const"] = const_cols(*pair(rng, 60, 50, 100))
    c["few_square"] = pair(rng, 48, 70, 48)
    z = feats(rng, 40, 96)
    c["few_same"] = (z, z.copy())
    c["few_tiny"] = pair(rng, 2, 2, 3)
    z1, z2 = pair(rng, 90, 80, 128)
    c["few_f32"] = (z1.astype(np.float32), z2.astype(np.float32))
    c["many_edge"] = pair(rng, 49, 70, 48)
    c["many_a"] = pair(rng, 300, 250, 40)
    z1, z2 = pair(rng, 200, 150, 48)
    g = np.exp(-0.2 * np.arange(48))
    c["many_graded"] = (z1 * g, z2 * g)
    c["many_const"] = const_cols(*pair(rng, 120, 90, 32))
    z = feats(rng, 150, 24)
    c["many_same"] = (z, z.copy())
    return c


def main():
    eu = load_eval_utils()
    d = {}
    cs = cases(np.random.default_rng(16))
    d["names"] = np.array(list(cs))
    for k, (z1, z2) in cs.items():
        few = k.startswith("few")
        assert (min(len(z1), len(z2)) <= z1.shape[1]) == few, k
        ref = float(eu.calculate_fid(z1, z2))
        lap, tr = fid_lapack(z1, z2)
        gap = abs(ref - lap)
        assert gap <= (1e-7 if few else 1e-12) * tr, (k, gap / tr)
        fid, _, sweeps, ok = fid_jacobi(z1, z2)
        assert ok and max(sweeps) <= 20, (k, sweeps)
        assert abs(fid - lap) <= 1e-12 * tr, (k, abs(fid - lap) / tr)
        d[f"{k}_z1"], d[f"{k}_z2"] = z1, z2
        d[f"{k}_ref"], d[f"{k}_lap"] = np.float64(ref), np.float64(lap)
        d[f"{k}_tr"], d[f"{k}_ref_gap"] = np.float64(tr), np.float64(gap)
        print(f"{k:12s} N1 {len(z1):4d} N2 {len(z2):4d} D {z1.shape[1]:4d} ref {ref:.17g} "
              f"lap {lap:.17g} ref_gap/tr {gap / tr:.2e} jacobi-lap/tr {abs(fid - lap) / tr:.2e} "
              f"sweeps {sweeps}")
    path = os.path.join(OUT, "g16_fid_device.npz")
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(f"wrote g16_fid_device.npz: {size} bytes")


if __name__ == "__main__":
    main()
