"""Trajectory distances of the flyability evaluation -- the functions of the reference's
evaluation/flyability_utils/trajectory_distances package (e_/s_ sspd, dtw, hausdorff, lcss,
erp, edr and discret_frechet) with the tables on the device.

The reference fills an (n0 + 1) x (n1 + 1) table per distance in a Python double loop, the
spherical ones with a sin / cos / atan2 chain per cell.  Here a whole list of pairs is packed
into one ragged batch, uploaded once, and csrc/tvq_traj.hip scores every pair in float64 with
one launch per kernel family:

  table    DTW, ERP, EDR, LCSS (Euclidean and spherical) and the discrete Frechet distance:
           nine recurrences over one anti-diagonal sweep (tvq_traj_table_distances, n >= 1)
  segment  SSPD and Hausdorff (Euclidean and spherical) from the per-point minima over the
           other trajectory's segments (tvq_traj_segment_distances, n >= 2)

The semantics are the reference's, quirks included: the spherical functions read column 0 as
the longitude and column 1 as the latitude whatever the caller put there, every ERP border
cell holds the total gap distance, EDR's borders are zero, `s_sspd` does not halve, and the
thresholds are compared with `cost < eps`.  A pair's row does not depend on the batch it is
in (bitwise).  There is no CPU fallback.

The continuous `frechet` (the reference's 14th distance) is apart from the 13 COLUMNS:
`frechet_device` scores a list of pairs with csrc/tvq_traj_frechet.hip (critical values,
sort and unique, binary search with a free-space decision per probe, all on the device) and
`frechet(P, Q)` is the reference's per-pair function."""
import numpy as np
import torch

from ...hip._native import call, ptr, stream_ptr, value
from .._device import resolve_device

COLUMNS = ("SSPD Euclidean", "SSPD Spherical", "DTW Euclidean", "DTW Spherical",
           "Hausdorff Euclidean", "Hausdorff Spherical", "LCSS Euclidean", "LCSS Spherical",
           "ERP Euclidean", "ERP Spherical", "EDR Euclidean", "EDR Spherical", "Discrete Frechet")
FAMILIES = ("table", "segment")


def max_len():
    """The longest trajectory the kernels accept (points)."""
    return int(value("tvq_traj_max_len"))


def _as_tensor(a, what, k, need):
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError(f"trajectory_distances: {what}[{k}] must be (n, 2), got {tuple(t.shape)}")
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"trajectory_distances: {what}[{k}] must be float32 or float64, "
                         f"got {t.dtype}")
    n = t.shape[0]
    if n < need:
        raise ValueError(f"trajectory_distances: {what}[{k}] has {n} point(s); "
                         + ("the segment metrics (SSPD, Hausdorff) need at least 2"
                            if need == 2 else "at least 1 is needed"))
    if n > max_len():
        raise ValueError(f"trajectory_distances: {what}[{k}] has {n} points, the kernels' limit "
                         f"is {max_len()}")
    return t.detach()


def _offsets(ts):
    return np.concatenate([[0], np.cumsum([t.shape[0] for t in ts])]).astype(np.int64)


def _pack(t0s, t1s, dev):
    """(pts0, off0, pts1, off1 on the device as float64 / int64; host off0, off1).  Host inputs
    travel as one buffer (both offset vectors, then the points in the inputs' widest dtype) and
    are widened on the device."""
    h0, h1 = _offsets(t0s), _offsets(t1s)
    n0, n1 = int(h0[-1]), int(h1[-1])
    head = torch.from_numpy(np.concatenate([h0, h1]))
    if all(not t.is_cuda for t in t0s + t1s):
        dt = torch.float64 if any(t.dtype == torch.float64 for t in t0s + t1s) else torch.float32
        body = torch.cat([t.to(dt).reshape(-1) for t in t0s + t1s])
        buf = torch.cat([head.view(torch.uint8), body.view(torch.uint8)]).to(dev)
        hb = head.numel() * 8
        offs = buf[:hb].view(torch.int64)
        pts = buf[hb:].view(dt).to(torch.float64)
    else:
        offs = head.to(dev)
        pts = torch.cat([t.to(dev).to(torch.float64).reshape(-1) for t in t0s + t1s])
    P1 = h0.size
    return (pts[:2 * n0], offs[:P1], pts[2 * n0:2 * (n0 + n1)], offs[P1:], h0, h1)


def _prepare(gen, sim, need):
    """The shared opening of the batch functions: (t0s, t1s), the checked tensors of two lists
    of equal length.  need: the fewest points a trajectory may have, or a function that returns
    it (and may refuse other arguments), called once the lengths are known to agree."""
    gen, sim = list(gen), list(sim)
    if len(gen) != len(sim):
        raise ValueError(f"trajectory_distances: {len(gen)} generated and {len(sim)} simulated "
                         f"trajectories")
    if callable(need):
        need = need()
    return ([_as_tensor(a, "gen", k, need) for k, a in enumerate(gen)],
            [_as_tensor(a, "sim", k, need) for k, a in enumerate(sim)])


def trajectory_distances_device(gen, sim, g, eps=0.009, lcss_spherical_eps=None,
                                edr_spherical_eps=None, device=None, families=FAMILIES):
    """(P, 13) float64 device tensor: row p holds the COLUMNS distances of (gen[p], sim[p]).

    gen, sim: equal-length lists of (n, 2) arrays or tensors (numpy or torch, CPU or CUDA,
    float32 or float64).  g: the ERP gap point.  eps: the threshold of Euclidean LCSS / EDR;
    spherical LCSS uses lcss_spherical_eps (default eps * 1e6) and spherical EDR
    edr_spherical_eps (default eps), as the reference's caller passes them.  families: which
    kernel families run; the columns of the other one are nan."""
    families = tuple(families)

    def need():
        if not families or any(f not in FAMILIES for f in families):
            raise ValueError(f"trajectory_distances: families must be chosen from {FAMILIES}")
        return 2 if "segment" in families else 1

    t0s, t1s = _prepare(gen, sim, need)
    g0, g1 = (float(v) for v in g)
    eps = float(eps)
    eps_ls = eps * 1e6 if lcss_spherical_eps is None else float(lcss_spherical_eps)
    eps_es = eps if edr_spherical_eps is None else float(edr_spherical_eps)
    dev = resolve_device(device, t0s + t1s)
    P = len(t0s)
    if P == 0:
        return torch.empty((0, len(COLUMNS)), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        pts0, off0, pts1, off1, h0, h1 = _pack(t0s, t1s, dev)
        out = torch.full((P, len(COLUMNS)), float("nan"), dtype=torch.float64, device=dev)
        if "table" in families:
            call("tvq_traj_table_distances", ptr(pts0), ptr(off0), ptr(pts1), ptr(off1),
                 h0.ctypes.data, h1.ctypes.data, P, g0, g1, eps, eps_ls, eps_es, ptr(out),
                 stream_ptr())
        if "segment" in families:
            call("tvq_traj_segment_distances", ptr(pts0), ptr(off0), ptr(pts1), ptr(off1),
                 h0.ctypes.data, h1.ctypes.data, P, ptr(out), stream_ptr())
    return out


def _one(column, family, t0, t1, g=(0.0, 0.0), **kw):
    out = trajectory_distances_device([t0], [t1], g, families=(family,), **kw)
    return float(out[0, COLUMNS.index(column)])


def e_sspd(t1, t2):
    return _one("SSPD Euclidean", "segment", t1, t2)


def s_sspd(t0, t1):
    return _one("SSPD Spherical", "segment", t0, t1)


def e_hausdorff(t1, t2):
    return _one("Hausdorff Euclidean", "segment", t1, t2)


def s_hausdorff(t0, t1):
    return _one("Hausdorff Spherical", "segment", t0, t1)


def e_dtw(t0, t1):
    return _one("DTW Euclidean", "table", t0, t1)


def s_dtw(t0, t1):
    return _one("DTW Spherical", "table", t0, t1)


def e_lcss(t0, t1, eps):
    return _one("LCSS Euclidean", "table", t0, t1, eps=eps)


def s_lcss(t0, t1, eps):
    return _one("LCSS Spherical", "table", t0, t1, lcss_spherical_eps=eps)


def e_erp(t0, t1, g):
    return _one("ERP Euclidean", "table", t0, t1, g=g)


def s_erp(t0, t1, g):
    return _one("ERP Spherical", "table", t0, t1, g=g)


def e_edr(t0, t1, eps):
    return _one("EDR Euclidean", "table", t0, t1, eps=eps)


def s_edr(t0, t1, eps):
    return _one("EDR Spherical", "table", t0, t1, edr_spherical_eps=eps)


def discret_frechet(t0, t1):
    return _one("Discrete Frechet", "table", t0, t1)


FRECHET_MAX_PAIRS = 65536  # pairs per tvq_traj_frechet call


def _frechet_bytes(h0, h1, a, b):
    """The workspace of pairs a..b-1, from the host offsets."""
    return int(value("tvq_traj_frechet_workspace", h0[a:].ctypes.data, h1[a:].ctypes.data, b - a))


def _frechet_chunks(h0, h1, budget):
    """[(a, b)]: consecutive runs of pairs, each the longest whose workspace fits `budget`."""
    P, chunks, a = h0.size - 1, [], 0
    while a < P:
        if _frechet_bytes(h0, h1, a, a + 1) > budget:
            raise ValueError(
                f"frechet: pair {a} ({h0[a + 1] - h0[a]} x {h1[a + 1] - h1[a]} points) needs a "
                f"workspace of {_frechet_bytes(h0, h1, a, a + 1)} bytes, workspace_bytes is "
                f"{budget}")
        lo, hi = a + 1, min(P, a + FRECHET_MAX_PAIRS)  # the workspace grows with the run
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if _frechet_bytes(h0, h1, a, mid) <= budget:
                lo = mid
            else:
                hi = mid - 1
        chunks.append((a, lo))
        a = lo
    return chunks


def frechet_device(gen, sim, device=None, workspace_bytes=1 << 30):
    """(P,) float64 device tensor: the continuous Frechet distance of (gen[p], sim[p]), the
    reference's trajectory_distances.frechet (csrc/tvq_traj_frechet.hip).

    gen, sim: as for trajectory_distances_device; a one-point trajectory is accepted (the
    result is the larger end-point distance).  The critical values of a pair, sorted on the
    device, take 32 (n0 - 1)(n1 - 1) bytes of workspace: the batch runs in chunks of
    consecutive pairs that fit `workspace_bytes`, and a single pair that does not is refused.
    A pair's value does not depend on the batch or the chunking (bitwise)."""
    t0s, t1s = _prepare(gen, sim, 1)
    chunks = _frechet_chunks(_offsets(t0s), _offsets(t1s), int(workspace_bytes))
    dev = resolve_device(device, t0s + t1s)
    P = len(t0s)
    if P == 0:
        return torch.empty((0,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        pts0, off0, pts1, off1, h0, h1 = _pack(t0s, t1s, dev)
        out = torch.full((P,), float("nan"), dtype=torch.float64, device=dev)
        need = max(_frechet_bytes(h0, h1, a, b) for a, b in chunks)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        for a, b in chunks:  # one stream: a chunk reuses the workspace after the one before
            call("tvq_traj_frechet", ptr(pts0), ptr(off0[a:]), ptr(pts1), ptr(off1[a:]),
                 h0[a:].ctypes.data, h1[a:].ctypes.data, b - a, ptr(out[a:]), ptr(ws), need,
                 stream_ptr())
    return out


def frechet(P, Q):
    """The continuous Frechet distance of one pair, as the reference's frechet.frechet."""
    return float(frechet_device([P], [Q])[0])
