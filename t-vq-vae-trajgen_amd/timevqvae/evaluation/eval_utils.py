"""FID and IS -- the API of the reference timevqvae/evaluation/eval_utils.py.

calculate_fid(z1, z2) (eval_utils.py:56-81): the feature means and sample covariances,
the O(N D^2) part, run on the device in float64 (tvq_fid_moments, csrc/tvq_fid.hip); the
D x D remainder -- sigma1 @ sigma2, its matrix square root (scipy.linalg.sqrtm, real part
when complex) and the trace -- stays on the host in float64 as in the reference.  That is the
default.  calculate_fid(..., sqrtm="device") / fid_device run the whole scalar on the device
instead (tvq_fid_device, csrc/tvq_fid.hip): tr sqrtm(sigma1 sigma2) is the sum of the
singular values of A1 A2^T, A_i = (z_i - mu_i) / sqrt(N_i - 1), found by one-sided Jacobi in
float64.

calculate_inception_score(P_yx, n_split, shuffle, eps) (eval_utils.py:9-53) is host numpy
over an (n, classes) probability table: the exp of the mean KL(p(y|x) || p(y)) per split.
"""
import numpy as np
import torch
from scipy.linalg import sqrtm as host_sqrtm

from ..hip._native import call, lib, ptr, stream_ptr, value
from ._device import resolve_device


def feature_moments(z, device=None):
    """(mu (D,), sigma (D, D)) of the rows of z (N, D): z.mean(0) and
    np.cov(z, rowvar=False), float64 on the device."""
    dev = resolve_device(device)
    zt = torch.as_tensor(z)
    if zt.dim() != 2 or zt.shape[0] < 2:
        raise ValueError("feature_moments: z must be (N >= 2, D)")
    zt = zt.to(device=dev, dtype=torch.float64).contiguous()
    N, D = zt.shape
    mu = torch.empty(D, device=dev, dtype=torch.float64)
    sigma = torch.empty(D, D, device=dev, dtype=torch.float64)
    call("tvq_fid_moments", ptr(zt), N, D, ptr(mu), ptr(sigma), stream_ptr())
    return mu, sigma


FID_FORMS = {"auto": 0, "few": 1, "many": 2}


def fid_device(z1, z2, device=None, form="auto", max_sweeps=40, return_parts=False):
    """calculate_fid wholly on the device in float64 (tvq_fid_device): a 0-dim float64 device
    tensor, NaN when a Jacobi run did not converge within max_sweeps sweeps; nothing is read
    back.  z1 (N1, D), z2 (N2, D): numpy or torch, CPU or CUDA, float32 or float64.  form
    "auto" takes "few" when min(N1, N2) <= D and "many" otherwise; either can be forced.
    return_parts adds (out (5,) float64 = fid, |mu1 - mu2|^2, tr sigma1, tr sigma2, T;
    info (5,) int32 = form used (1 few, 2 many), sweeps of the sigma1 / sigma2 / W runs,
    converged), both on the device."""
    if form not in FID_FORMS:
        raise ValueError(f"fid_device: form must be one of {sorted(FID_FORMS)}, got {form!r}")
    dev = resolve_device(device)
    zs = [torch.as_tensor(z) for z in (z1, z2)]
    if any(z.dim() != 2 or z.shape[0] < 2 for z in zs) or zs[0].shape[1] != zs[1].shape[1]:
        raise ValueError("fid_device: z1, z2 must be (N1 >= 2, D) and (N2 >= 2, D)")
    zs = [z.to(device=dev, dtype=torch.float64).contiguous() for z in zs]
    (N1, D), N2 = zs[0].shape, zs[1].shape[0]
    nbytes = value("tvq_fid_device_workspace", N1, N2, D, FID_FORMS[form])
    if nbytes < 0:
        raise ValueError("fid_device: " + lib().tvq_last_error().decode())
    out = torch.empty(5, device=dev, dtype=torch.float64)
    info = torch.empty(5, device=dev, dtype=torch.int32)
    ws = torch.empty(int(nbytes), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        call("tvq_fid_device", ptr(zs[0]), N1, ptr(zs[1]), N2, D, FID_FORMS[form], int(max_sweeps),
             ptr(out), ptr(info), ptr(ws), stream_ptr())
    return (out[0], out, info) if return_parts else out[0]


def calculate_fid(z1, z2, device=None, sqrtm="host"):
    """Frechet distance between the Gaussian fits of two feature sets (rows = samples).
    sqrtm="host" is the reference's scipy.linalg.sqrtm of sigma1 @ sigma2; "device" is
    float(fid_device(z1, z2, device)) and raises RuntimeError when it did not converge."""
    if sqrtm not in ("host", "device"):
        raise ValueError(f"calculate_fid: sqrtm must be 'host' or 'device', got {sqrtm!r}")
    if sqrtm == "device":
        fid = float(fid_device(z1, z2, device))
        if fid != fid:
            raise RuntimeError("calculate_fid(sqrtm='device'): the Jacobi sweeps did not converge")
        return fid
    mu1, sigma1 = feature_moments(z1, device)
    mu2, sigma2 = feature_moments(z2, device)
    mu1, mu2 = mu1.cpu().numpy(), mu2.cpu().numpy()
    sigma1, sigma2 = sigma1.cpu().numpy(), sigma2.cpu().numpy()
    ssdiff = ((mu1 - mu2) ** 2.0).sum()
    covmean = host_sqrtm(sigma1.dot(sigma2))
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    return ssdiff + np.trace(sigma1 + sigma2 - 2.0 * covmean)


def calculate_inception_score(P_yx, n_split: int = 10, shuffle: bool = True, eps: float = 1e-16):
    """(mean, std) over n_split splits of exp(E_x KL(p(y|x) || p(y))); shuffles P_yx in
    place with np.random first when `shuffle` (as the reference does)."""
    if shuffle:
        np.random.shuffle(P_yx)
    n_part = int(np.floor(P_yx.shape[0] / n_split))
    scores = []
    for i in range(n_split):
        part = P_yx[i * n_part:(i + 1) * n_part]
        p_y = part.mean(axis=0)[None, :]
        kl = (part * (np.log(part + eps) - np.log(p_y + eps))).sum(axis=1)
        scores.append(np.exp(np.mean(kl)))
    return np.mean(scores), np.std(scores)
