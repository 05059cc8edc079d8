"""The RMSNorm / LayerNorm row-norm kernels (csrc/tvq_rownorm.hip), every dispatch arm of the
forward and the backward against torch autograd in fp64 on the CPU.

D picks the arm: 8 and 32 the backward's 32-lanes-per-row form (RMSNorm; with and without
dead lanes), 48 / 64 one element per lane, 100 / 128 two, 200 / 256 four (ragged, full), 320
the one-wave-per-row loop; the ragged widths and 320 also take the non-vector forward.  M
picks the row bookkeeping (norm_rows_per_block: max(4, ceil(M / 256)) rows per block): 1 is
one block of one row, every other slot prefetching the clamped row; 5 a second block of one
row; 1031 is 5 rows per block (a wave's second trip with a real prefetch, idle slots in the
32-lane form, a last block of one row); 2300 is 9 rows per block, 256 blocks, the last of 5
rows (two wave-uniform trips of the 32-lane form, half a wave dead on the second).

Bound: relative L2 error < 1e-5 for y, dx and every parameter gradient, the tolerance of
tests/test_stage2.py::test_rmsnorm_layernorm.  An fp32 emulation of both backward passes with
fully sequential row sums (a worse order than the kernels') stays <= 1.2e-6 on the gain and
bias gradients and < 1e-7 on dx at these shapes; one row dropped of 2300 moves a gain gradient
by about 2e-2."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DS = [8, 32, 48, 64, 100, 128, 200, 256, 320]
MS = [1, 5, 1031, 2300]
CASES = ["rms", "rms_res", "ln_gb", "ln_g", "ln"]
TOL = 1e-5


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def arm(case, D):
    """The backward TVQ_PLAN line of a case at width D."""
    op = "rmsnorm" if case.startswith("rms") else "layernorm"
    if D > 256:
        return f"{op}_bwd loop"
    if op == "rmsnorm" and D <= 32:
        return f"{op}_bwd LR32 ND1"
    return f"{op}_bwd LR64 ND{1 if D <= 64 else 2 if D <= 128 else 4}"


def inputs(case, D, M):
    """CPU fp32 inputs: x, the output gradient(s) and the case's parameters by name."""
    gen = torch.Generator().manual_seed(1000 * D + M)
    x = torch.randn(M, D, generator=gen) * 3 + 0.5
    gy = torch.randn(M, D, generator=gen)
    gr = torch.randn(M, D, generator=gen) if case == "rms_res" else None
    params = {}
    if case != "ln":
        params["g"] = torch.rand(D, generator=gen) + 0.5
    if case == "ln_gb":
        params["b"] = torch.randn(D, generator=gen)
    return x, gy, gr, params


def reference(case, D, x, gy, gr, params):
    x = x.double().requires_grad_(True)
    p = {k: v.double().requires_grad_(True) for k, v in params.items()}
    if case.startswith("rms"):
        y = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12) * D ** 0.5 * p["g"]
    else:
        y = F.layer_norm(x, (D,), p.get("g"), p.get("b"), 1e-5)
    y.backward(gy.double())
    dx = x.grad if gr is None else x.grad + gr.double()
    return {"y": y, "dx": dx, **{"d" + k: v.grad for k, v in p.items()}}


def preset_grad(n):
    return torch.sin(torch.arange(n, device="cuda", dtype=torch.float32))


def device_run(case, D, x, gy, gr, params, accumulate):
    """Forward + backward on the HIP path -> (results by name, the backward's plan lines).
    accumulate: the parameters carry preset .grad buffers the backward kernels add into
    (hip._native.grad_sink), as FusedAdamW's flat gradient does."""
    from timevqvae.hip._native import plan_trace
    from timevqvae.hip.xf import layer_norm, rmsnorm, rmsnorm_res
    xd = x.cuda().requires_grad_(True)
    p = {k: v.cuda().requires_grad_(True) for k, v in params.items()}
    if accumulate:
        for v in p.values():
            v._tvq_flat = True
            v.grad = preset_grad(D)
    sinks = {k: v.grad.data_ptr() for k, v in p.items()} if accumulate else {}
    if case == "rms":
        outs, gouts = [rmsnorm(xd, p["g"])], [gy.cuda()]
    elif case == "rms_res":
        outs, gouts = list(rmsnorm_res(xd, p["g"])), [gy.cuda(), gr.cuda()]
    else:
        outs, gouts = [layer_norm(xd, p.get("g"), p.get("b"), 1e-5)], [gy.cuda()]
    with plan_trace() as tr:
        torch.autograd.backward(outs, gouts)
    torch.cuda.synchronize()
    for k, v in p.items():  # no Python-side gradient: .grad is still the preset buffer
        assert not accumulate or v.grad.data_ptr() == sinks[k]
    res = {"y": outs[0], "dx": xd.grad, **{"d" + k: v.grad for k, v in p.items()}}
    return res, [t for t in tr.lines if t.startswith(("rmsnorm_bwd", "layernorm_bwd"))]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("D", DS)
def test_rownorm_vs_fp64(D, M, case):
    x, gy, gr, params = inputs(case, D, M)
    ref = reference(case, D, x, gy, gr, params)
    got, lines = device_run(case, D, x, gy, gr, params, accumulate=False)
    assert lines == [arm(case, D)], lines
    assert sorted(got) == sorted(ref)
    for k in ref:
        e = rel(got[k], ref[k])
        print(f"{case} D{D} M{M} {k}: {e:.2e}")
        assert e < TOL, (k, e)
    # a second run on the same inputs: bitwise equal
    again, _ = device_run(case, D, x, gy, gr, params, accumulate=False)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    # accumulate = 1: preset + gradient in the parameters' own buffers
    acc, lines = device_run(case, D, x, gy, gr, params, accumulate=True)
    assert lines == [arm(case, D)], lines
    for k in ref:
        want = ref[k] + preset_grad(D).double().cpu() if k in ("dg", "db") else ref[k]
        e = rel(acc[k], want)
        print(f"{case} D{D} M{M} {k} (accumulate): {e:.2e}")
        assert e < TOL, (k, e)
