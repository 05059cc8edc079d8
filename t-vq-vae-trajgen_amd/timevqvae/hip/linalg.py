"""One-sided Jacobi singular values (tvq_jacobi_sv, csrc/tvq_fid.hip): the kernel under
evaluation.fid_device, exposed alone so it can be tested alone."""
import torch

from ._native import call, ptr, stream_ptr, value


def jacobi_sv(a, m_dot=None, max_sweeps=40):
    """Orthogonalise the rows of a (n, m_all) float64 device tensor IN PLACE by Hestenes
    rotations; the first m_dot (default m_all) entries of each row enter the inner products
    and the rotation decisions.  Returns (sigma (n,) float64: the rows' 2-norms over m_dot
    entries, unsorted, all NaN when not converged; info (2,) int32: sweeps that ran,
    converged 0 / 1), both on the device; nothing is read back."""
    if a.dim() != 2 or a.dtype != torch.float64 or not a.is_contiguous():
        raise ValueError("jacobi_sv: a must be a contiguous (n, m_all) float64 tensor")
    n, m_all = a.shape
    m_dot = m_all if m_dot is None else int(m_dot)
    sigma = torch.empty(n, device=a.device, dtype=torch.float64)
    info = torch.empty(2, device=a.device, dtype=torch.int32)
    nbytes = value("tvq_jacobi_sv_workspace", n)
    ws = torch.empty(max(int(nbytes), 8), device=a.device, dtype=torch.uint8)
    with torch.cuda.device(a.device):
        call("tvq_jacobi_sv", ptr(a), n, m_all, m_dot, int(max_sweeps), ptr(sigma), ptr(info),
             ptr(ws), stream_ptr())
    return sigma, info
