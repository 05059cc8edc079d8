"""The MaskGIT prior's glue kernels (timevqvae.hip.xf over csrc/tvq_xf.hip, tvq_dropout_bwd of
csrc/tvq_norm.hip, tvq_layer_drop of csrc/tvq_train.hip, the attention of csrc/tvq_attn.hip),
op by op, against the same expression in torch on the CPU in float64 with gradients by
autograd, the same inputs and the same upstream gradient.

Bounds
  Floating-point results (CE gradients, GELU, attention, the embedding's table gradient):
  the bound of test_fe_train_ops.py, per tensor and elementwise |got - ref64| <= 1e-5
  max|ref64| + 1e-4 |ref64|, and rel-L2 <= 1e-5.  Every case first requires float32 CPU torch
  to stay within a quarter of that bound, so a badly conditioned input fails as a test-input
  error and not as a kernel error.  Where the reference tensor is exactly zero (dq and dk at
  S = 1: a softmax over one key is constant) there is no magnitude to divide by and the
  kernel's tensor must be exactly zero.
  Pure data movement (gathers, scatters of single values, concatenation, index choices,
  masks) is compared with torch.equal.  A kept element of a dropout is x * (1 / (1 - p)), the
  scale computed in float32 (one subtraction, one division) and one product: within
  3 * 2^-24 |ref64| of the float64 product; a dropped element is exactly zero.
  Short ordered sums (upsample_nearest's backward, batch_colsum, dpos): a float32 sum of m
  terms in any order lies within (m - 1) 2^-24 sum|terms| of the exact sum; sum|terms| comes
  from the same float64 reference applied to |dy|.  Two calls must agree bit for bit.

Dropout masks are rebuilt on the host from the documented counter hash (tvq_common.h
mix_seed / uniform01, restated by test_stage2._hash_uniform): seed = rng.seed_tensor, offset
= what rng.call_offset(site) hands the call, keep = U(seed, offset, counter) >= p.

Shapes: the smallest that reach the path named, and the constant in the source that puts
them there (move the case when the constant moves).
  embedding (embedding_fwd_kernel, grid_for's cap of 8192 blocks of 256 = 2 097 152 elements;
  the group-by of tvq_reduce.hip: one-block sort up to GB1_MAX_M = 2048 rows, 128-row
  chunks of seg_sum_kernel; counter m D + d):
    (V 33, D 128, M 500) one-block sort; (513, 128, 16500) M D = 2 112 000 > 2 097 152, the
    forward's stride loop, and M > 2048, the three-launch sort; (514, 64, 3000) the mask
    token owns 60 % of the rows = 1800 rows = 15 chunks of 128 rows, combined in chunk order,
    and its rows are undropped; (6, 48, 37) D below a wave and no multiple of 64.
  masked CE (masked_ce_fwd_kernel: tvq_masked_ce_workspace caps the grid at 1024 blocks of 4
  waves, one row per wave = 4096 rows; masked_ce_bwd_kernel: grid_for, 2 097 152 elements):
    (M 4100, K 513) both stride loops (M K = 2 103 300), its last four rows masked;
    (7, 33) K < 64, under two blocks; (130, 64) K = one wave's stride, logits x 30 (peaked);
    (9, 1025) K = 16 strides + 1; (64, 2) K = 2; one masked row placed last; 64 leading rows
    kept (16 blocks whose four waves all skip); ldl = K + 3 and ldd = K + 2 through the C
    entry point.  With every row kept the loss is 0 / 0, as in torch; no case expects it.
  embed_assemble (grid_for, 2 097 152 elements; batch_colsum8_kernel for dpos):
    (B 5, n 7, D1 12, D2 0) the LF form; (3, 13, 20, 12) t1 a transposed view, dt1 written
    through its strides; (170, 96, 64, 64) B (n + 1) Dt = 2 110 720 > 2 097 152.
  drop_first_token (float4 lanes; grid_for on float4 units): (3, 2, 4) one float4 a row;
    (5, 26, 128); (700, 97, 128) 700 * 96 * 32 = 2 150 400 float4 > 2 097 152.
  batch_colsum (BCS_PARTS = 8 batch parts, BCS_COLS = 32 columns a block): B = 1, 7 (< 8),
    9 and 33 (no multiples of 8), 256; n D = 15, 70, 32 and 12312 (ragged last block).
  upsample_nearest (grid_for): up by 2, ragged up, Lin > 128, a downsample with unmapped
    inputs, Lin = 1, (R 4200, 256 -> 512) R Lout = 2 150 400 > 2 097 152.  Transposed form
    (tvq_upsample_nearest_t_bwd: the tile kernel for Lin <= 128, 64-channel tiles UPT_D):
    D = 70 at Lin = 128 (ragged second tile), Lin = 129 (the per-element kernel), the
    downsample and Lin = 1.
  gelu, dropout (grid caps 8192 x 256): n = 1, 255 / 257 (around one block), 2 100 000.
  scale_by (float4, 2048 blocks x 256 x 4 = 2 097 152 elements): n = 4, 1028, 2 100 004.
  class_index (256-thread blocks): B = 1, 257, 1000.  layer_drop (one block, n <= 256).
  attention (ATT tiles of 32 rows, S <= 128): S = 32 one full tile, 65 two tiles + 1, 127
    one short of four, 1, 97 with inputs x 2; (2, 33, 2) through qkv_attention (ld = 3 H 64)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_stage2 import _hash_uniform

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MASK64 = 0xFFFFFFFFFFFFFFFF


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ratio(t, ref, tol):
    d = (t.double() - ref).abs()
    r = torch.where(tol > 0, d / tol.clamp_min(1e-300), torch.where(d > 0, math.inf, 0.0))
    return float(r.max())


def _check(got, ref64, ref32, what):
    """The module bound for one tensor; the float32 CPU reference must use <= 1/4 of it."""
    got = got.detach().cpu()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    if float(ref64.abs().max()) == 0.0:  # no magnitude: exactly zero
        assert not ref32.any(), f"{what}: test input: float32 torch is not exactly zero"
        print(f"{what}: reference exactly zero, kernel max |.| {float(got.abs().max()):.3e}")
        assert not got.any(), f"{what}: {float(got.abs().max()):.3e} where the reference is zero"
        return
    tol = 1e-5 * ref64.abs().max() + 1e-4 * ref64.abs()
    r32, rk = _ratio(ref32, ref64, tol), _ratio(got, ref64, tol)
    rel = float((got.double() - ref64).norm() / (ref64.norm() + 1e-30))
    print(f"{what}: kernel {rk:.3f} / float32 torch {r32:.3f} of the bound, rel-L2 {rel:.2e}")
    assert r32 <= 0.25, f"{what}: test input: float32 torch at {r32:.3f} of the bound"
    assert rk <= 1.0, f"{what}: {rk:.3f} of the bound"
    assert rel <= 1e-5, f"{what}: rel-L2 {rel:.3e}"


def _check_sum(got, ref64, abs64, m, what):
    """The ordered-sum bound: |got - exact| <= (m - 1) 2^-24 sum|terms| (m a number or a
    tensor of per-element term counts)."""
    got = got.detach().cpu()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    m1 = torch.as_tensor(m, dtype=torch.float64) - 1
    tol = m1.clamp_min(0) * U * abs64
    r = _ratio(got, ref64, tol)
    print(f"{what}: {r:.3f} of the summation-order bound")
    assert r <= 1.0, f"{what}: {r:.3f} of the summation-order bound"


def _check_scaled(got, ref64, what):
    """One float32 product by a float32 scale: 3 roundings; zero where the reference is."""
    got = got.detach().cpu()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    r = _ratio(got, ref64, 3 * U * ref64.abs())
    print(f"{what}: {r:.3f} of three roundings")
    assert r <= 1.0, f"{what}: {r:.3f} of three roundings"


def _ref(fn, inputs, gy, dtype):
    """fn's value and its gradients w.r.t. every non-None input, on the CPU in `dtype`."""
    xs = [None if t is None else t.detach().to(dtype).requires_grad_() for t in inputs]
    y = fn(*xs)
    gs = torch.autograd.grad(y, [x for x in xs if x is not None], gy.to(dtype))
    return y.detach(), gs


def _dev(fn, inputs, gy, cuda):
    xs = [None if t is None else t.detach().to(cuda).requires_grad_() for t in inputs]
    y = fn(*xs)
    gs = torch.autograd.grad(y, [x for x in xs if x is not None], gy.to(cuda))
    torch.cuda.synchronize()
    return y.detach(), gs


def _check_all(fn_hip, fn_ref, inputs, gy, names, cuda):
    y64, g64 = _ref(fn_ref, inputs, gy, torch.float64)
    y32, g32 = _ref(fn_ref, inputs, gy, torch.float32)
    yd, gd = _dev(fn_hip, inputs, gy, cuda)
    _check(yd, y64, y32, "fwd")
    assert len(gd) == len(names)
    for got, r64, r32, n in zip(gd, g64, g32, names):
        _check(got, r64, r32, n)
    return yd, gd


def _p32(p):
    """p as the kernels see it (a float argument), as a Python float."""
    return float(np.float32(p))


def _next_offset(site):
    """The offset rng.call_offset(site) hands the next call."""
    from timevqvae.hip import rng
    return (site + rng._calls[0] + 1) & MASK64


def _seed(cuda):
    from timevqvae.hip import rng
    return int(rng.seed_tensor(cuda).item())


def _hash_u(seed, offset, n):
    """U(seed, offset, i), i < n, as float32 (exact: multiples of 2^-24)."""
    u = _hash_uniform(seed, offset, np.arange(n, dtype=np.uint64))
    return torch.from_numpy(u.astype(np.float32))


def _hash_keep(seed, offset, n, p):
    return _hash_u(seed, offset, n) >= torch.tensor(p, dtype=torch.float32)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------- embedding with dropout
def _emb_idx(V, M, kind, gen):
    idx = torch.randint(0, V, (M,), generator=gen)
    if kind == "skewed":  # the mask token (V - 1) owns 60 % of the rows
        hot = torch.rand(M, generator=gen) < 0.6
        idx = torch.where(hot, torch.full_like(idx, V - 1), idx)
    return idx


EMB_CASES = [(33, 128, 500, "uniform", 32, 0.3), (513, 128, 16500, "uniform", 512, 0.3),
             (514, 64, 3000, "skewed", 513, 0.3), (6, 48, 37, "uniform", 5, 0.3),
             (33, 128, 500, "uniform", -1, 0.3),  # mask_id = -1: dropout everywhere
             (33, 128, 500, "uniform", 7, 0.0)]   # p = 0: mask_id is inert


@pytest.mark.parametrize("V,D,M,kind,mask_id,p", EMB_CASES)
def test_embedding_dropout(V, D, M, kind, mask_id, p, cuda):
    """Forward = table[idx] keep / (1 - p) with the hash mask at counter m D + d and the
    mask token's rows undropped bit for bit; the table gradient (autograd, and the C entry
    point accumulating onto a non-zero table) is the float64 index_add of g keep / (1 - p)
    with the same mask."""
    from timevqvae.hip import rng
    from timevqvae.hip._native import call, ptr, stream_ptr, value
    from timevqvae.hip.xf import embedding
    gen = _gen(V * 1000 + M + (mask_id & 0xFF))
    idx = _emb_idx(V, M, kind, gen)
    table, g, t0 = (torch.randn(s, generator=gen) for s in ((V, D), (M, D), (V, D)))
    site = 91 << 40
    seed, off = _seed(cuda), _next_offset(site)
    exempt = (idx == mask_id)[:, None].expand(M, D) if p > 0 else torch.ones(M, D, dtype=torch.bool)
    if p > 0:
        keep = _hash_keep(seed, off, M * D, p).reshape(M, D) | exempt
        if mask_id >= 0:
            assert (idx == mask_id).any() and (idx != mask_id).any()
        assert 0.6 < float(keep[idx != mask_id].float().mean()) < 0.8
    else:
        keep = torch.ones(M, D, dtype=torch.bool)
    # the mask token's rows are neither dropped nor scaled
    w64 = torch.where(exempt, 1.0, keep.double() / (1.0 - _p32(p)))
    tabd = table.to(cuda).requires_grad_()
    idd, gd = idx.to(cuda), g.to(cuda)
    out = embedding(idd, tabd, mask_id, p, site)
    if p > 0:
        assert rng._calls[0] + site == off, "the call took the offset the mask was built from"
    (dt,) = torch.autograd.grad(out, [tabd], gd)
    torch.cuda.synchronize()
    out = out.detach().cpu()
    assert torch.equal(out == 0, ~keep | (table[idx] == 0)), "the dropped set is the hash mask's"
    _check_scaled(out, table[idx].double() * w64, "fwd")
    same = (idx == mask_id) if p > 0 else torch.ones(M, dtype=torch.bool)
    assert torch.equal(_bits(out[same]), _bits(table[idx[same]])), "undropped rows are the table's"
    r64 = torch.zeros(V, D, dtype=torch.float64).index_add(0, idx, g.double() * w64)
    r32 = torch.zeros(V, D).index_add(0, idx, g * w64.float())
    _check(dt, r64, r32, "dtable")
    # accumulate = 1 onto a non-zero table gradient, same seed and offset
    tg = t0.to(cuda)
    ws = torch.empty(value("tvq_embedding_bwd_workspace", M, V), device=cuda, dtype=torch.int32)
    call("tvq_embedding_bwd", ptr(idd), M, D, ptr(gd), D, V, ptr(tg), 1, mask_id, p,
         ptr(rng.seed_tensor(cuda)), off, ptr(ws), stream_ptr())
    torch.cuda.synchronize()
    _check(tg, t0.double() + r64, t0 + r32, "dtable0 + dtable")


# ---------------------------------------------------------------- masked cross-entropy
def _ce_inputs(M, K, scale, kept, seed):
    gen = _gen(seed)
    logits = scale * torch.randn(M, K, generator=gen)
    target = torch.randint(0, K, (M,), generator=gen)
    keep = torch.rand(M, generator=gen) < kept
    return logits, target, keep


def _ce_ref(logits, target, keep, dtype):
    lg = logits.detach().to(dtype).requires_grad_()
    loss = F.cross_entropy(lg[~keep], target[~keep])
    (dl,) = torch.autograd.grad(loss, [lg])
    return loss.detach(), dl


def _ce_check(logits, target, keep, cuda):
    from timevqvae.hip.xf import masked_cross_entropy
    n_masked = int((~keep).sum())
    assert n_masked > 0
    l64, d64 = _ce_ref(logits, target, keep, torch.float64)
    l32, d32 = _ce_ref(logits, target, keep, torch.float32)
    lgd = logits.to(cuda).requires_grad_()
    loss = masked_cross_entropy(lgd, target.to(cuda), keep.to(cuda))
    stats = loss.grad_fn.saved_tensors[4]
    (dl,) = torch.autograd.grad(loss, [lgd])
    torch.cuda.synchronize()
    e, e32 = abs(float(loss) - float(l64)), abs(float(l32) - float(l64))
    print(f"loss: kernel {e / (1e-5 * abs(float(l64))):.3f} / float32 torch "
          f"{e32 / (1e-5 * abs(float(l64))):.3f} of 1e-5 relative")
    assert e32 <= 0.25e-5 * abs(float(l64)), "test input: float32 torch loss"
    assert e <= 1e-5 * abs(float(l64)), (float(loss), float(l64))
    assert float(stats[1]) == n_masked, (float(stats[1]), n_masked)
    _check(dl, d64, d32, "dlogits")
    assert not dl.cpu()[keep].any(), "dlogits is exactly zero on kept rows"


@pytest.mark.parametrize("M,K,scale,kept", [(4100, 513, 3.0, 0.5), (7, 33, 3.0, 0.5),
                                            (130, 64, 30.0, 0.7), (9, 1025, 3.0, 0.1),
                                            (64, 2, 1.0, 0.5)])
def test_masked_ce(M, K, scale, kept, cuda):
    logits, target, keep = _ce_inputs(M, K, scale, kept, M * 10 + K)
    if M > 4096:
        keep[4096:] = False  # the rows only the forward's second stride reaches are masked
    assert keep.any()
    _ce_check(logits, target, keep, cuda)


def test_masked_ce_one_masked_row_last(cuda):
    logits, target, keep = _ce_inputs(7, 33, 3.0, 0.5, 11)
    keep[:] = True
    keep[-1] = False
    _ce_check(logits, target, keep, cuda)


def test_masked_ce_whole_blocks_kept(cuda):
    """Rows 0..63 kept: 16 blocks of the forward whose four waves all skip."""
    logits, target, keep = _ce_inputs(130, 64, 30.0, 0.7, 12)
    keep[:64] = True
    keep[64:68] = False
    _ce_check(logits, target, keep, cuda)


def test_masked_ce_leading_dimensions(cuda):
    """tvq_masked_ce_fwd / bwd with the logits a column slice of a wider buffer (ldl = K + 3)
    and dlogits padded (ldd = K + 2): the pad columns keep their sentinel."""
    from timevqvae.hip._native import call, ptr, stream_ptr, value
    M, K = 37, 33
    logits, target, keep = _ce_inputs(M, K, 3.0, 0.5, 13)
    l64, d64 = _ce_ref(logits, target, keep, torch.float64)
    l32, d32 = _ce_ref(logits, target, keep, torch.float32)
    wide = torch.full((M, K + 3), 1e4)
    wide[:, 2:2 + K] = logits
    wide = wide.to(cuda)
    lg = wide[:, 2:]
    assert lg.data_ptr() == wide.data_ptr() + 8 and lg.stride(0) == K + 3
    td, kd = target.to(cuda), keep.to(cuda)
    lse, out = torch.empty(M, device=cuda), torch.empty(2, device=cuda)
    ws = torch.empty(value("tvq_masked_ce_workspace", M), device=cuda)
    call("tvq_masked_ce_fwd", ptr(lg), K + 3, M, K, ptr(td), ptr(kd), ptr(lse), ptr(out), ptr(ws),
         stream_ptr())
    dl = torch.full((M, K + 2), 7.5, device=cuda)
    gout = torch.ones(1, device=cuda)
    call("tvq_masked_ce_bwd", ptr(lg), K + 3, M, K, ptr(td), ptr(kd), ptr(lse), ptr(out), ptr(gout),
         ptr(dl), K + 2, stream_ptr())
    torch.cuda.synchronize()
    assert abs(float(out[0]) - float(l64)) <= 1e-5 * abs(float(l64))
    assert float(out[1]) == int((~keep).sum())
    _check(dl[:, :K], d64, d32, "dlogits")
    assert not dl.cpu()[:, :K][keep].any()
    assert bool((dl[:, K:] == 7.5).all()), "the pad columns of dlogits are not written"


# ---------------------------------------------------------------- embed_assemble
def _asm_inputs(B, n, D1, D2, transposed, seed):
    gen = _gen(seed)
    Dt = D1 + D2
    cls = torch.randn(B, 1, Dt, generator=gen)
    t1 = torch.randn(B, D1, n, generator=gen) if transposed else torch.randn(B, n, D1, generator=gen)
    t2 = torch.randn(B, n, D2, generator=gen) if D2 else None
    pos = torch.randn(n + 3, Dt, generator=gen)
    g = torch.randn(B, n + 1, Dt, generator=gen)
    p0 = torch.randn(n + 3, Dt, generator=gen)
    return cls, t1, t2, pos, g, p0


ASM_CASES = [(5, 7, 12, 0, False), (3, 13, 20, 12, True), (170, 96, 64, 64, False)]


@pytest.mark.parametrize("accumulate", [False, True], ids=["plain", "accumulate"])
@pytest.mark.parametrize("B,n,D1,D2,transposed", ASM_CASES)
def test_embed_assemble(B, n, D1, D2, transposed, accumulate, cuda):
    """cat([cls, cat([t1, t2], -1) + pos[:n]], 1): forward exact (one float32 add, as torch's);
    dcls, dt1 (through t1's strides) and dt2 are slices of g; dpos[:n] is g's batch sum within
    the ordered-sum bound, rows >= n untouched; plain (autograd) and accumulate (onto the
    position table's non-zero flat gradient) modes."""
    from timevqvae.hip.xf import embed_assemble
    cls, t1, t2, pos, g, p0 = _asm_inputs(B, n, D1, D2, transposed, B * 100 + n)
    view = (lambda t: t.transpose(1, 2)) if transposed else (lambda t: t)
    tok = view(t1) if t2 is None else torch.cat([view(t1), t2], -1)
    want = torch.cat([cls, tok + pos[:n]], 1)
    outs = []
    for _ in range(2):
        cd, b1, pd = (t.to(cuda).requires_grad_() for t in (cls, t1, pos))
        b2 = t2.to(cuda).requires_grad_() if t2 is not None else None
        if accumulate:  # as FusedAdamW keeps it: the kernel adds into pos.grad
            pd._tvq_flat = True
            pd.grad = p0.to(cuda)
        t1d = view(b1)
        y = embed_assemble(cd, t1d, b2, pd, n)
        assert torch.equal(y.detach().cpu(), want)
        seen = []  # dt1 as the op hands it to autograd (.grad of a view is re-laid out)
        t1d.register_hook(lambda gr: seen.append((gr.stride(), gr.detach().cpu())))
        y.backward(g.to(cuda))
        torch.cuda.synchronize()
        assert torch.equal(cd.grad.cpu(), g[:, :1])
        assert len(seen) == 1 and torch.equal(seen[0][1], g[:, 1:, :D1])
        assert seen[0][0] == t1d.stride(), "dt1 carries t1's strides"
        assert torch.equal(b1.grad.cpu(), view(g[:, 1:, :D1]))
        if t2 is not None:
            assert torch.equal(b2.grad.cpu(), g[:, 1:, D1:])
        outs.append(pd.grad.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "dpos is bitwise repeatable"
    base = p0 if accumulate else torch.zeros_like(p0)
    ref = base.double()
    ref[:n] += g[:, 1:].double().sum(0)
    s = base.double().abs()
    s[:n] += g[:, 1:].double().abs().sum(0)
    assert torch.equal(_bits(outs[0][n:]), _bits(base[n:])), "rows >= n get no gradient"
    _check_sum(outs[0], ref, s, B + int(accumulate), "dpos")


# ---------------------------------------------------------------- drop_first_token
@pytest.mark.parametrize("B,n1,D", [(3, 2, 4), (5, 26, 128), (700, 97, 128)])
def test_drop_first_token(B, n1, D, cuda):
    from timevqvae.hip.xf import drop_first_token
    gen = _gen(B + n1)
    x, g = torch.randn(B, n1, D, generator=gen), torch.randn(B, n1 - 1, D, generator=gen)
    xd = x.to(cuda).requires_grad_()
    y = drop_first_token(xd)
    assert y.grad_fn is not None and type(y.grad_fn).__name__.startswith("_DropFirst")
    (dx,) = torch.autograd.grad(y, [xd], g.to(cuda))
    torch.cuda.synchronize()
    assert y.is_contiguous() and torch.equal(_bits(y), _bits(x[:, 1:]))
    want = torch.cat([torch.zeros(B, 1, D), g], 1)  # row 0 is +0.0
    assert torch.equal(_bits(dx), _bits(want))


# ---------------------------------------------------------------- batch_colsum
@pytest.mark.parametrize("accumulate", [False, True], ids=["plain", "accumulate"])
@pytest.mark.parametrize("pad", [0, 1], ids=["ldo=D", "ldo=D+1"])
@pytest.mark.parametrize("B,n,D", [(1, 3, 5), (7, 3, 5), (9, 24, 513), (256, 1, 70), (33, 2, 16)])
def test_batch_colsum(B, n, D, pad, accumulate, cuda):
    from timevqvae.hip.xf import batch_colsum
    gen = _gen(B * 1000 + n * D)
    x = torch.randn(B, n, D, generator=gen)
    o0 = torch.randn(n, D + pad, generator=gen)
    o0[:, D:] = 7.5
    xd = x.to(cuda)
    outs = []
    for _ in range(2):
        out = o0.to(cuda)
        batch_colsum(xd, out, D + pad, accumulate)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "bitwise repeatable"
    assert bool((outs[0][:, D:] == 7.5).all()), "the pad column is not written"
    ref, s = x.double().sum(0), x.double().abs().sum(0)
    if accumulate:
        ref, s = ref + o0[:, :D].double(), s + o0[:, :D].double().abs()
    _check_sum(outs[0][:, :D], ref, s, B + int(accumulate), "colsum")


# ---------------------------------------------------------------- upsample_nearest
def _src_index(Lin, Lout):
    """min(floor(float32(j) * float32(Lin / Lout)), Lin - 1), as torch and the kernels have
    it; checked against F.interpolate's own gather on the CPU (the input check)."""
    scale = np.float32(Lin) / np.float32(Lout)
    j = np.arange(Lout, dtype=np.float32)
    src = torch.from_numpy(np.minimum(np.floor(j * scale), Lin - 1).astype(np.int64))
    probe = torch.arange(Lin, dtype=torch.float32).reshape(1, 1, Lin)
    assert torch.equal(F.interpolate(probe, size=Lout, mode="nearest").reshape(-1).long(), src), \
        "test input: the float32 source index differs from F.interpolate's"
    return src


def _up_check(y, dx, x, gy, src, Lin, what):
    """x (R, Lin), gy (R, Lout) on the CPU; y, dx the kernel's."""
    assert torch.equal(_bits(y), _bits(x[:, src])), f"{what}: forward"
    R = x.shape[0]
    ref = torch.zeros(R, Lin, dtype=torch.float64).index_add_(1, src, gy.double())
    s = torch.zeros(R, Lin, dtype=torch.float64).index_add_(1, src, gy.double().abs())
    cnt = torch.bincount(src, minlength=Lin)
    dx = dx.detach().cpu()
    assert not dx[:, cnt == 0].any(), f"{what}: exactly zero where no output maps"
    assert not torch.signbit(dx[:, cnt == 0]).any()
    _check_sum(dx, ref, s, cnt[None, :].expand(R, Lin), f"{what} dx")


UP_CASES = [(6, 16, 32), (4, 25, 97), (3, 130, 300), (2, 97, 25), (5, 1, 9), (4200, 256, 512)]


@pytest.mark.parametrize("R,Lin,Lout", UP_CASES)
def test_upsample_nearest(R, Lin, Lout, cuda):
    from timevqvae.hip.xf import upsample_nearest
    src = _src_index(Lin, Lout)
    if Lin > Lout:
        assert (torch.bincount(src, minlength=Lin) == 0).any()
    gen = _gen(Lin * 1000 + Lout)
    x, gy = torch.randn(R, Lin, generator=gen), torch.randn(R, Lout, generator=gen)
    xd = x.to(cuda).requires_grad_()
    y = upsample_nearest(xd, Lout)
    (dx,) = torch.autograd.grad(y, [xd], gy.to(cuda))
    (dx2,) = torch.autograd.grad(upsample_nearest(xd, Lout), [xd], gy.to(cuda))
    torch.cuda.synchronize()
    assert torch.equal(_bits(dx), _bits(dx2)), "bitwise repeatable"
    _up_check(y, dx, x, gy, src, Lin, "upsample_nearest")


# the tile kernel (Lin <= 128) with a ragged second channel tile (D = 70 > UPT_D = 64); the
# per-element kernel (Lin = 129); a downsample and Lin = 1 (both in the tile kernel)
@pytest.mark.parametrize("B,Lin,D,Lout", [(2, 128, 70, 300), (2, 129, 70, 300), (2, 97, 16, 25),
                                          (3, 1, 8, 9)])
def test_upsample_nearest_t(B, Lin, D, Lout, cuda):
    from timevqvae.hip.xf import upsample_nearest_t
    src = _src_index(Lin, Lout)
    gen = _gen(Lin * 1000 + Lout + D)
    x, gy = torch.randn(B, Lin, D, generator=gen), torch.randn(B, D, Lout, generator=gen)
    xd = x.to(cuda).requires_grad_()
    y = upsample_nearest_t(xd, Lout)
    (dx,) = torch.autograd.grad(y, [xd], gy.to(cuda))
    (dx2,) = torch.autograd.grad(upsample_nearest_t(xd, Lout), [xd], gy.to(cuda))
    torch.cuda.synchronize()
    assert torch.equal(_bits(dx), _bits(dx2)), "bitwise repeatable"
    assert tuple(y.shape) == (B, D, Lout) and tuple(dx.shape) == (B, Lin, D)
    rows = lambda t: t.detach().cpu().transpose(1, 2).reshape(B * D, -1)  # (B, L, D) -> rows
    _up_check(y.detach().cpu().reshape(B * D, Lout), rows(dx), rows(x), gy.reshape(B * D, Lout),
              src, Lin, "upsample_nearest_t")


# ---------------------------------------------------------------- GELU, scale_by
def _gelu_check(x, gy, cuda):
    from timevqvae.hip.xf import gelu
    _check_all(gelu, F.gelu, [x], gy, ["dx"], cuda)


def test_gelu_values(cuda):
    """5000 normal draws x 3 and the edges: signed zeros, the tails where erf saturates
    (+-6, +-10, +-40) and a denormal-product input."""
    gen = _gen(21)
    x = torch.cat([3 * torch.randn(5000, generator=gen),
                   torch.tensor([0.0, -0.0, 6.0, -6.0, 10.0, -10.0, 40.0, -40.0, 1e-30])])
    gy = torch.randn(x.shape, generator=gen)
    _gelu_check(x, gy, cuda)
    from timevqvae.hip.xf import gelu
    y = gelu(x.to(cuda)).cpu()
    assert torch.isfinite(y).all() and float(y[5000]) == 0.0 and float(y[5001]) == 0.0
    assert float(y[5006]) == 40.0 and float(y[5007]) == 0.0


@pytest.mark.parametrize("n", [1, 255, 257, 2_100_000])
def test_gelu_sizes(n, cuda):
    gen = _gen(22 + n)
    _gelu_check(3 * torch.randn(n, generator=gen), torch.randn(n, generator=gen), cuda)


@pytest.mark.parametrize("n", [4, 1028, 2_100_004])
def test_scale_by(n, cuda):
    from timevqvae.hip.linear import scale_by
    gen = _gen(n)
    x, s = torch.randn(n, generator=gen), torch.randn(1, generator=gen)
    y = scale_by(x.to(cuda), s.to(cuda))
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(x * s))


# ---------------------------------------------------------------- class index
def _class_index(y, p, null, cuda, rnd=None, seed=None, off=0):
    from timevqvae.hip._native import call, ptr, stream_ptr
    yd = y.to(cuda)
    idx = torch.empty_like(yd)
    rd = rnd.to(cuda) if rnd is not None else None
    call("tvq_class_index", ptr(yd), y.numel(), p, null, ptr(seed), off, ptr(rd), ptr(idx),
         stream_ptr())
    torch.cuda.synchronize()
    return idx.cpu()


@pytest.mark.parametrize("B", [1, 257, 1000])
def test_class_index_injected_draws(B, cuda):
    """idx = where(u > p, y, null) (the reference's bidirectional_transformer.py:142), with u
    exactly at p, one float32 below and one above."""
    p, null = 0.2, 5
    p32 = torch.tensor(p, dtype=torch.float32)
    edges = torch.stack([p32, torch.nextafter(p32, torch.tensor(0.0)),
                         torch.nextafter(p32, torch.tensor(1.0))])
    gen = _gen(B)
    y = torch.randint(0, null, (B,), generator=gen)
    for k in range(3 if B == 1 else 1):
        u = torch.rand(B, generator=gen)
        if B == 1:
            u[0] = edges[k]
        else:
            u[3:6], u[B - 3:] = edges, edges
        want = torch.where(u > p32, y, torch.full_like(y, null))
        got = _class_index(y, p, null, cuda, rnd=u)
        assert torch.equal(got, want)
        if B > 1:
            assert want[3:6].tolist() == [null, null, int(y[5])]


def test_class_index_device_draws(cuda):
    from timevqvae.hip import rng
    B, p, null = 1000, 0.2, 5
    y = torch.randint(0, null, (B,), generator=_gen(3))
    off = (93 << 40) + 17
    u = _hash_u(_seed(cuda), off, B)
    want = torch.where(u > torch.tensor(p, dtype=torch.float32), y, torch.full_like(y, null))
    assert 0.1 < float((want == null).float().mean()) < 0.3
    got = _class_index(y, p, null, cuda, seed=rng.seed_tensor(cuda), off=off)
    assert torch.equal(got, want)


# ---------------------------------------------------------------- layer_drop, dropout
@pytest.mark.parametrize("n", [1, 8, 256])
def test_layer_drop(n, cuda):
    """keep[i] = U(seed, offset, i) >= p; touched = keep (accumulate = 0, overwriting a mixed
    pattern) or max(touched, keep) (accumulate = 1)."""
    from timevqvae.hip import rng
    from timevqvae.hip._native import call, ptr, stream_ptr
    p = 0.3
    for k, off in enumerate(((94 << 40) + 1, (94 << 40) + 2, (95 << 40) + 1)):
        want = _hash_keep(_seed(cuda), off, n, p).float()
        pattern = (torch.arange(n) % 2 == k % 2).float()
        for accumulate in (0, 1):
            keep = torch.full((n,), -1.0, device=cuda)
            touched = pattern.to(cuda)
            call("tvq_layer_drop", ptr(rng.seed_tensor(cuda)), off, p, n, ptr(keep), ptr(touched),
                 accumulate, stream_ptr())
            torch.cuda.synchronize()
            assert torch.equal(keep.cpu(), want), (off, accumulate)
            assert torch.equal(touched.cpu(), torch.maximum(pattern, want) if accumulate else want)
    if n > 1:
        u = _hash_keep(_seed(cuda), (94 << 40) + 1, 256, p)
        assert 0.55 < float(u.float().mean()) < 0.85


@pytest.mark.parametrize("n", [1, 1000, 2_100_000])
def test_dropout(n, cuda):
    """dropout(x, p, site) = x keep / (1 - p) with the hash mask at counter i; the backward
    applies the same mask to the gradient."""
    from timevqvae.hip import rng
    from timevqvae.models.bidirectional_transformer import dropout
    p, site = 0.3, 96 << 40
    gen = _gen(n)
    x, gy = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    off = _next_offset(site)
    keep = _hash_keep(_seed(cuda), off, n, p)
    xd = x.to(cuda).requires_grad_()
    y = dropout(xd, p, site)
    assert rng._calls[0] + site == off
    (dx,) = torch.autograd.grad(y, [xd], gy.to(cuda))
    torch.cuda.synchronize()
    w64 = keep.double() / (1.0 - _p32(p))
    for got, src, what in ((y, x, "fwd"), (dx, gy, "dx")):
        got = got.detach().cpu()
        assert torch.equal(got == 0, ~keep | (src == 0)), f"{what}: the dropped set is the hash mask's"
        _check_scaled(got, src.double() * w64, what)
    if n > 1:
        assert 0.6 < float(keep.float().mean()) < 0.8


# ---------------------------------------------------------------- attention
def _attn_ref(H, keep=None, p=0.0):
    def fn(q, k, v):
        B, S, _ = q.shape
        sh = lambda t: t.reshape(B, S, H, 64).transpose(1, 2)
        a = torch.softmax(sh(q) @ sh(k).transpose(-1, -2) / 8.0, -1)
        if keep is not None:
            a = a * keep.to(a.dtype) / (1.0 - p)
        return (a @ sh(v)).transpose(1, 2).reshape(B, S, H * 64)
    return fn


# one full tile; two tiles and a row; one short of four tiles; one key (dq = dk = 0); the
# sharpened softmax (inputs x 2; x 4 leaves float32 torch over a quarter of the bound)
@pytest.mark.parametrize("B,S,H,scale", [(2, 32, 1, 1.0), (2, 65, 2, 1.0), (1, 127, 1, 1.0),
                                         (3, 1, 2, 1.0), (2, 97, 1, 2.0)])
def test_attention(B, S, H, scale, cuda):
    from timevqvae.hip.xf import attention
    gen = _gen(S * 10 + H)
    q, k, v = (scale * torch.randn(B, S, H * 64, generator=gen) for _ in range(3))
    go = torch.randn(B, S, H * 64, generator=gen)
    _check_all(lambda q_, k_, v_: attention(q_, k_, v_, H), _attn_ref(H), [q, k, v], go,
               ["dq", "dk", "dv"], cuda)


def test_qkv_attention(cuda):
    """q, k, v as column blocks of one stacked projection (ld = 3 H 64): the output, dx and
    the three projection weights' gradients against softmax((x Wq)(x Wk)^T / 8)(x Wv)."""
    from timevqvae.hip.xf import qkv_attention
    B, S, H, D = 2, 33, 2, 128
    gen = _gen(33)
    x = torch.randn(B, S, D, generator=gen)
    wq, wk, wv = (torch.randn(H * 64, D, generator=gen) / math.sqrt(D) for _ in range(3))
    go = torch.randn(B, S, H * 64, generator=gen)
    core = _attn_ref(H)
    _check_all(lambda x_, q_, k_, v_: qkv_attention(x_, q_, k_, v_, H),
               lambda x_, q_, k_, v_: core(x_ @ q_.T, x_ @ k_.T, x_ @ v_.T),
               [x, wq, wk, wv], go, ["dx", "dWq", "dWk", "dWv"], cuda)


def test_attention_dropout_hash_mask(cuda):
    """keep(q, k) = U(seed, offset, (bh S + q) S + k) >= p scaled by 1 / (1 - p), forward and
    backward, at two full tiles plus one row."""
    from timevqvae.hip import rng
    from timevqvae.hip.xf import attention
    B, S, H, p, site = 2, 65, 2, 0.3, 97 << 40
    gen = _gen(65)
    q, k, v, go = (torch.randn(B, S, H * 64, generator=gen) for _ in range(4))
    off = _next_offset(site)
    keep = _hash_keep(_seed(cuda), off, B * H * S * S, p).reshape(B, H, S, S)
    _check_all(lambda q_, k_, v_: attention(q_, k_, v_, H, drop_p=p, site=site),
               _attn_ref(H, keep, _p32(p)), [q, k, v], go, ["dq", "dk", "dv"], cuda)
    assert rng._calls[0] + site == off
