"""A numpy statement of the device FID (csrc/tvq_fid_sqrt.hip): one-sided Jacobi singular
values with round-robin pairing, the "few" and "many" forms of tr sqrtm(sigma1 sigma2), and
the LAPACK form of the same scalar.  Shared by tests/golden/make_golden_fid_device.py (which
asserts convergence on every fixture case) and tests/test_fid_device.py.  It states the
algorithm, not the summation order: results agree with the device to rounding, not bit for
bit."""
import numpy as np

EPS = 2.0 ** -52


def round_pairs(n, r):
    """The disjoint pairs (p, q) of round r of the chess tournament on n players: n - 1 rounds
    for even n, n rounds with one bye each for odd n."""
    ne = n + (n & 1)
    k = np.arange(ne // 2)
    p = np.where(k == 0, ne - 1, (r + k) % (ne - 1))
    q = np.where(k == 0, r, (r - k + ne - 1) % (ne - 1))
    keep = (p < n) & (q < n)
    return p[keep], q[keep]


def jacobi_sv(a, m_dot=None, max_sweeps=40):
    """Orthogonalise the rows of a (n, m_all) in place; the first m_dot entries decide.
    Returns (norms over m_dot entries, sweeps run, converged)."""
    n, m_all = a.shape
    m_dot = m_all if m_dot is None else m_dot
    thr = EPS * np.sqrt(float(m_dot))
    ne = n + (n & 1)
    sweeps, rotated = 0, 1
    while sweeps < max_sweeps and rotated:
        rotated = 0
        for r in range(ne - 1 if n > 1 else 0):
            p, q = round_pairs(n, r)
            ap, aq = a[p, :m_dot], a[q, :m_dot]
            alpha, beta = (ap * ap).sum(1), (aq * aq).sum(1)
            gamma = (ap * aq).sum(1)
            with np.errstate(all="ignore"):
                go = (alpha != 0) & (beta != 0) & (
                    np.abs(gamma) > thr * (np.sqrt(alpha) * np.sqrt(beta)))
                zeta = (beta - alpha) / (2.0 * gamma)
                t = np.where(zeta == 0, 1.0, np.sign(zeta) / (np.abs(zeta) + np.hypot(1.0, zeta)))
            t = np.where(go, t, 0.0)
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = c * t
            # c x_p - s x_q and s x_p + c x_q in Rutishauser's form, tau = s / (1 + c): for a
            # small angle c rounds to 1 (always upwards), which would inflate every norm
            tau = s / (1.0 + c)
            p, q, s, tau = p[go], q[go], s[go, None], tau[go, None]
            xp, xq = a[p], a[q]
            a[p], a[q] = xp - s * (xq + tau * xp), xq + s * (xp - tau * xq)
            rotated += int(go.sum())
        sweeps += 1
    nrm = np.sqrt((a[:, :m_dot] ** 2).sum(1))
    return nrm, sweeps, rotated == 0


def centred(z):
    z = np.asarray(z, np.float64)
    mu = z.mean(0)
    return mu, (z - mu) / np.sqrt(z.shape[0] - 1.0)


def psd_factor(sigma, max_sweeps=40):
    """F with rows sqrt(lambda_j) v_j^T (F^T F = sigma) from Jacobi on the stack [sigma ; I]."""
    D = sigma.shape[0]
    st = np.concatenate([sigma, np.eye(D)], 1)
    lam, sweeps, ok = jacobi_sv(st, D, max_sweeps)
    return np.sqrt(lam)[:, None] * st[:, D:], sweeps, ok


def fid_jacobi(z1, z2, form="auto", max_sweeps=40):
    """(fid, tr sigma1 + tr sigma2, sweeps of the Jacobi runs, converged)."""
    mu1, a1 = centred(z1)
    mu2, a2 = centred(z2)
    D = a1.shape[1]
    if form == "auto":
        form = "few" if min(a1.shape[0], a2.shape[0]) <= D else "many"
    ssdiff = ((mu1 - mu2) ** 2).sum()
    if form == "few":
        w = a1 @ a2.T if a1.shape[0] <= a2.shape[0] else a2 @ a1.T
        tr1, tr2 = (a1 * a1).sum(), (a2 * a2).sum()
        sv, sw, ok = jacobi_sv(np.ascontiguousarray(w), None, max_sweeps)
        sweeps = (0, 0, sw)
    else:
        s1, s2 = a1.T @ a1, a2.T @ a2
        tr1, tr2 = np.trace(s1), np.trace(s2)
        f1, sw1, ok1 = psd_factor(s1, max_sweeps)
        f2, sw2, ok2 = psd_factor(s2, max_sweeps)
        sv, sw3, ok3 = jacobi_sv(f1 @ f2.T, None, max_sweeps)
        sweeps, ok = (sw1, sw2, sw3), ok1 and ok2 and ok3
    fid = ssdiff + tr1 + tr2 - 2.0 * sv.sum() if ok else np.nan
    return fid, tr1 + tr2, sweeps, ok


def fid_lapack(z1, z2):
    """(fid, tr sigma1 + tr sigma2) with T = the sum of LAPACK's singular values of A1 A2^T."""
    mu1, a1 = centred(z1)
    mu2, a2 = centred(z2)
    tr = (a1 * a1).sum() + (a2 * a2).sum()
    t = np.linalg.svd(a1 @ a2.T, compute_uv=False).sum()
    return ((mu1 - mu2) ** 2).sum() + tr - 2.0 * t, tr
