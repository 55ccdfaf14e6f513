"""The backward of the Gaussian-mixture prior (layers/autograd.py: gmm_backward / _gmm_param_part, seven launches) against
torch.autograd in fp64, at every branch of its kernels' launch plans and with responsibilities that are genuinely mixed.

GPU tests go through the C ABI like tests/test_gpu_parity.py; the reference is torch.autograd through the fp64 CPU oracle
(oracle.flow_oracle.gmm_logprob) on the same inputs, and for cf_gmm_resp the closed form of tests/helpers.py.  The bar is the
project's rule for gradients (test_backward_against_autograd_oracle): per tensor, max|got - ref| / max(max|ref|, 1e-3) below
max(1e-4, 3 x the error fp32 torch.autograd makes on the same graph and inputs); the fp32 floor is computed on the CPU from
the reference code alone.  Measured errors of the product next to these floors: profiles/gmm_backward_errors.md."""
import math
import types

import pytest
import torch

from oracle import flow_oracle as fo
from tests.helpers import gmm_resp_closed_form

DEV = "cuda:0"

# (M, K, D, B, row stride of x) and what each is the smallest shape to reach:
#   (10, 8, 768, 300, 1536)   three sample tiles (the last ragged), a channel slice, 12 d-slices in tree + tail order,
#                             cf_gmm_bwd_sums with ragged batch slices
#   (10, 8, 1536, 70, 1536)   one tile, 24 slices
#   (10, 8, 99, 131, 99)      D % 4 != 0 (scalar loads); D % 32 != 0: the cf_linear_wgrad / _x2 fallback; a ragged last d-chunk
#   (10, 8, 48, 257, 48)      no split (ns = 1) through the split-form kernel; fallback sums
#   (10, 8, 96, 4, 128)       a batch smaller than one k-step of the sums kernel, on a slice
#   (10, 8, 64, 5, 1 << 20)   row stride at the xbs < 2^20 limit: fallback with a non-contiguous x (the copy branch)
#   (1, 5, 64, 200, 64)       M K = 5 <= 16 (one component per thread), 51 samples per finish block, M = 1
#   (33, 8, 256, 40, 256)     M K = 264 > 256: four component blocks, k_gmm_resp_finish
#   (2, 8, 1536, 1400, 1536)  B D = 2 150 400 > 8192 x 256: the grid-stride wrap of k_gmm_bwd_gx
#   (33, 8, 8192, 3, 8192)    M K D = 2 162 688 > 8192 x 256: the wrap of k_gmm_bwd_coeffs and k_gmm_bwd_params; 64 d-slices
CASES = [(10, 8, 768, 300, 1536), (10, 8, 1536, 70, 1536), (10, 8, 99, 131, 99), (10, 8, 48, 257, 48), (10, 8, 96, 4, 128),
         (10, 8, 64, 5, 1 << 20), (1, 5, 64, 200, 64), (33, 8, 256, 40, 256), (2, 8, 1536, 1400, 1536), (33, 8, 8192, 3, 8192)]
IDS = ["-".join(map(str, c)) for c in CASES]
EW_BLOCKS = 8192 * 256                      # elements one pass of the elementwise kernels' grids covers (gmm_ew_blocks)


@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


# ------------------------------------------------------------------------------------------ inputs and references (CPU)
def _overlap_case(M, K, D, B, seed):
    """Mixture parameters whose components overlap, samples drawn from the mixtures themselves, an upstream gradient.
    The K means of a mixture lie 1/sqrt(D) per coordinate around a common centre and their scales differ by a relative
    0.5/sqrt(D): the log-joints of a mixture's components then differ by O(1) for every D - the responsibilities are mixed,
    not one-hot.  Returns fp32 (x (B, D), mG, sG (M, K, D), wG (M, K), g (B, M))."""
    gen = torch.Generator().manual_seed(seed)
    rs = 1.0 / math.sqrt(D)
    c = torch.randn(M, 1, D, generator=gen)
    mG = c + torch.randn(M, K, D, generator=gen) * rs
    sigma = (0.5 + torch.rand(M, 1, D, generator=gen)) * (1.0 + 0.5 * torch.randn(M, K, D, generator=gen) * rs)
    sG = torch.log(torch.expm1(sigma))
    wG = torch.randn(M, K, generator=gen)
    mb, kb = torch.randint(0, M, (B,), generator=gen), torch.randint(0, K, (B,), generator=gen)
    x = mG[mb, kb] + sigma[mb, kb] * torch.randn(B, D, generator=gen)
    g = torch.randn(B, M, generator=gen)
    return x, mG, sG, wG, g


def _autograd_reference(x, mG, sG, wG, g, dtype, chunk=64):
    """Gradients of sum(g * log p) with respect to (x, mG, sG, wG) by torch.autograd through the oracle in `dtype`: forward and
    backward per chunk of samples, the gradients accumulating in the leaves (chunk = None: one graph over the whole batch)."""
    lx, lm, ls, lw = [t.to(dtype).clone().requires_grad_(True) for t in (x, mG, sG, wG)]
    gd = g.to(dtype)
    B = x.shape[0]
    step = B if chunk is None else chunk
    for b0 in range(0, B, step):
        lp = fo.gmm_logprob(lx[b0:b0 + step], lm, ls, lw, chunk=step)
        (lp * gd[b0:b0 + step]).sum().backward()
    return {"gx": lx.grad, "mG": lm.grad, "sG": ls.grad, "wG": lw.grad}


def _rel_err(got, ref):
    return (got.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3)


_case_cache = {}


def _case(case):
    """Inputs of a CASES entry and its fp64 responsibilities (B, M, K), computed once and never written to; the references of
    the GPU tests come from _with_references."""
    if case not in _case_cache:
        M, K, D, B, stride = case
        x, mG, sG, wG, g = _overlap_case(M, K, D, B, 1000 * D + B)
        d = lambda t: t.double()
        resp = gmm_resp_closed_form(d(x), d(mG), d(sG), d(wG), torch.ones(B, M, dtype=torch.float64)).view(B, M, K)
        _case_cache[case] = types.SimpleNamespace(x=x, mG=mG, sG=sG, wG=wG, g=g, resp=resp, ref=None, floor=None)
    return _case_cache[case]


def _with_references(case):
    """The case with ref = fp64 autograd gradients (gx, mG, sG, wG) and the closed-form r, and floor = the relative error the
    same code makes in fp32 - computed once, shared by the GPU tests."""
    c = _case(case)
    if c.ref is None:
        d = lambda t: t.double()
        ref = _autograd_reference(c.x, c.mG, c.sG, c.wG, c.g, torch.float64)
        ref["r"] = gmm_resp_closed_form(d(c.x), d(c.mG), d(c.sG), d(c.wG), d(c.g))
        f32 = _autograd_reference(c.x, c.mG, c.sG, c.wG, c.g, torch.float32)
        f32["r"] = gmm_resp_closed_form(c.x, c.mG, c.sG, c.wG, c.g)
        c.floor = {k: _rel_err(f32[k], ref[k]) for k in ref}
        c.ref = ref
    return c


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_overlap_condition(case):
    """The responsibilities of the inputs are mixed: in at least 40 % of the (b, m) pairs the largest fp64 responsibility is
    below 0.9 (independent randn parameters at these D give 0 %: log-joints hundreds apart, a softmax of zeros and a one)."""
    c = _case(case)
    share = (c.resp.max(-1).values < 0.9).double().mean().item()
    print("GMM_OVERLAP %s share of (b, m) with max_k responsibility < 0.9: %.3f" % ("-".join(map(str, case)), share))
    assert torch.isfinite(c.resp).all()
    assert (c.resp.sum(-1) - 1.0).abs().max().item() < 1e-12
    assert share >= 0.4, share


def test_chunked_reference_equals_unchunked():
    """The per-chunk forward + backward with accumulating leaves is the gradient of the whole batch: 1e-12 relative at 130
    samples (two whole chunks and a ragged third)."""
    x, mG, sG, wG, g = _overlap_case(3, 4, 20, 130, 7)
    a = _autograd_reference(x, mG, sG, wG, g, torch.float64, chunk=64)
    b = _autograd_reference(x, mG, sG, wG, g, torch.float64, chunk=None)
    for k in a:
        err = (a[k] - b[k]).abs().max().item() / b[k].abs().max().item()
        assert err < 1e-12, (k, err)


def test_closed_form_responsibilities_are_the_gradient_of_the_log_joints():
    """The closed form of cf_gmm_resp against autograd: r = d sum(g * logsumexp_k lj) / d lj, i.e. the gradient of the oracle's
    log-probability with respect to wG before its log-softmax, per sample - checked through sum_b r = d/d logw."""
    x, mG, sG, wG, g = [t.double() for t in _overlap_case(3, 4, 20, 130, 7)]
    r = gmm_resp_closed_form(x, mG, sG, wG, g)
    logw = torch.log_softmax(wG, -1).requires_grad_(True)
    sig = torch.nn.functional.softplus(sG)
    lj = (-0.5 * ((x.view(-1, 1, 1, 20) - mG) / sig) ** 2 - torch.log(sig) - 0.5 * math.log(2 * math.pi)).sum(-1) + logw
    (torch.logsumexp(lj, -1) * g).sum().backward()
    err = (r.sum(0).view(3, 4) - logw.grad).abs().max().item() / logw.grad.abs().max().item()
    assert err < 1e-12, err


# ------------------------------------------------------------------------------------------ GPU
def _device_x(c, case):
    """x on the device as the last D columns of a (B, stride) tensor (seeded filler in front: a read through the wrong stride
    finds other numbers, not zeros)."""
    M, K, D, B, stride = case
    if stride == D:
        return c.x.to(DEV)
    wide = torch.empty(B, stride, device=DEV)
    wide.normal_(generator=torch.Generator(device=DEV).manual_seed(B))
    wide[:, stride - D:] = c.x.to(DEV)
    return wide[:, stride - D:]


def _bar(c, key, got, case, what):
    err, floor = _rel_err(got.detach().cpu(), c.ref[key]), c.floor[key]
    tol = max(1e-4, 3.0 * floor)
    print("GMM_BWD %s %s %s: relative error %.3e, fp32 floor %.3e, bar %.3e" % (what, "-".join(map(str, case)), key, err, floor, tol))
    return err, floor, tol


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gmm_backward_against_fp64(L, case):
    """autograd.gmm_backward - cf_gmm_resp, cf_gmm_bwd_coeffs, two cf_linear, cf_gmm_bwd_gx, cf_gmm_bwd_sums or the
    cf_linear_wgrad / _x2 pair, cf_gmm_bwd_params_w - against fp64 autograd through the oracle: gx and the gradients of mG, sG
    and wG, each under the bar of the module docstring.  The same call with the column sums of g supplied, and with
    params=False, gives the same gx bit for bit.  (Measured: profiles/gmm_backward_errors.md.)"""
    from contextflow_amd.layers import autograd
    from contextflow_amd.layers.distributions.gaussian import gmm_prepare
    M, K, D, B, stride = case
    c = _with_references(case)
    x = _device_x(c, case)
    assert x.stride(0) == stride or B == 1
    dist = types.SimpleNamespace(mG=c.mG.to(DEV), sG=c.sG.to(DEV), wG=c.wG.to(DEV))
    prep = gmm_prepare(dist.mG, dist.sG, dist.wG)
    g = c.g.to(DEV)
    gx, gp = autograd.gmm_backward(x, dist, prep, g)
    torch.cuda.synchronize()
    assert gx.shape == (B, D) and gx.dtype == torch.float32
    got = {"gx": gx, "mG": gp[dist.mG], "sG": gp[dist.sG], "wG": gp[dist.wG]}
    assert got["mG"].shape == (M, K, D) and got["sG"].shape == (M, K, D) and got["wG"].shape == (M, K)
    fails = []
    for key, t in got.items():
        assert torch.isfinite(t).all(), key
        err, floor, tol = _bar(c, key, t, case, "backward")
        if not err < tol:
            fails.append("%s: relative error %.3e (fp32 floor %.3e, bar %.1e)" % (key, err, floor, tol))
    assert not fails, fails
    gx2, gp2 = autograd.gmm_backward(x, dist, prep, g, gcol=g.sum(0))
    assert torch.equal(gx2, gx)
    for p in (dist.mG, dist.sG, dist.wG):                 # g.sum(0) is what the call forms itself when gcol is None
        assert torch.equal(gp2[p], gp[p])
    gx3, none = autograd.gmm_backward(x, dist, prep, g, params=False)
    assert none is None and torch.equal(gx3, gx)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gmm_resp_against_fp64(L, case):
    """cf_gmm_resp called directly: r (B, M K) against softmax_k(log-joint + log_softmax(wG)) * g[b, m] in fp64; the floor is
    the same closed form in fp32."""
    from contextflow_amd.layers import _hip
    from contextflow_amd.layers.distributions.gaussian import gmm_prepare
    M, K, D, B, stride = case
    c = _with_references(case)
    x = _device_x(c, case)
    a, nm, cst, _, _, _ = gmm_prepare(c.mG.to(DEV), c.sG.to(DEV), c.wG.to(DEV))
    g = c.g.to(DEV)
    r = torch.full((B, M * K), float("nan"), device=DEV)
    ws = torch.empty(_hip.lib().cf_gmm_resp_ws_bytes(B, M, K, D), device=DEV, dtype=torch.uint8)
    _hip.call("cf_gmm_resp", _hip.p(x), _hip.p(a), _hip.p(nm), _hip.p(cst), _hip.p(g), _hip.p(r), _hip.p(ws), B, M, K, D, stride,
              _hip.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(r).all()
    err, floor, tol = _bar(c, "r", r, case, "resp")
    assert err < tol, "r: relative error %.3e (fp32 floor %.3e, bar %.1e)" % (err, floor, tol)


def _ulp(ref):
    """Spacing of the fp32 numbers at |ref| (ref fp64, normal range)."""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(ref), e - 24)


@pytest.mark.gpu
@pytest.mark.parametrize("MK,D", [(80, 96), (264, 8192)])
def test_gmm_backward_elementwise_entries(L, MK, D):
    """cf_gmm_bwd_coeffs, both layouts: A2 = a a (one rounding) and AB = (a a) nm (two) within 2 ulp of the exact products, the
    transposed outputs the transposes of the plain ones bit for bit.  cf_gmm_bwd_params = the mG / sG outputs of
    cf_gmm_bwd_params_w on the same sums, bit for bit.  (264, 8192): 2 162 688 elements, past one pass of the 8192-block grid.
    Every output starts as NaN: an element no thread wrote stays one."""
    from contextflow_amd.layers import _hip
    pp, st = _hip.p, _hip.stream()
    n = MK * D
    assert (n > EW_BLOCKS) == (D == 8192)
    gen = torch.Generator().manual_seed(MK + D)
    a = (0.5 + 1.5 * torch.rand(MK, D, generator=gen))
    nm = torch.randn(MK, D, generator=gen)
    nm = torch.where(nm.abs() < 1e-3, torch.full_like(nm, 0.5), nm)            # products stay in the normal range
    ad, nd = a.to(DEV), nm.to(DEV)
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    A2, AB, A2t, ABt = nan(MK, D), nan(MK, D), nan(D, MK), nan(D, MK)
    _hip.call("cf_gmm_bwd_coeffs", pp(ad), pp(nd), pp(A2), pp(AB), MK, D, 0, st)
    _hip.call("cf_gmm_bwd_coeffs", pp(ad), pp(nd), pp(A2t), pp(ABt), MK, D, 1, st)
    torch.cuda.synchronize()
    a64, n64 = a.double(), nm.double()
    for got, ref in ((A2, a64 * a64), (AB, a64 * a64 * n64)):
        assert torch.isfinite(got).all()
        worst = ((got.cpu().double() - ref).abs() / _ulp(ref)).max().item()
        assert worst <= 2.0, worst
    assert torch.equal(A2t, A2.t()) and torch.equal(ABt, AB.t())
    # the parameter kernel with and without the mixture-weight part
    K = 8
    M = MK // K
    sG, S1, S2 = torch.randn(MK, D, generator=gen).to(DEV), torch.randn(MK, D, generator=gen).to(DEV), torch.rand(MK, D, generator=gen).to(DEV)
    S0, wG, gcol = torch.randn(MK, generator=gen).to(DEV), torch.randn(M, K, generator=gen).to(DEV), torch.randn(M, generator=gen).to(DEV)
    gmu, gsig, gmu_w, gsig_w, gw = nan(MK, D), nan(MK, D), nan(MK, D), nan(MK, D), nan(M, K)
    _hip.call("cf_gmm_bwd_params", pp(ad), pp(nd), pp(sG), pp(S0), pp(S1), pp(S2), pp(gmu), pp(gsig), MK, D, st)
    _hip.call("cf_gmm_bwd_params_w", pp(ad), pp(nd), pp(sG), pp(S0), pp(S1), pp(S2), pp(wG), pp(gcol), pp(gmu_w), pp(gsig_w), pp(gw),
              M, K, D, st)
    torch.cuda.synchronize()
    assert torch.isfinite(gmu).all() and torch.isfinite(gsig).all() and torch.isfinite(gw).all()
    assert torch.equal(gmu, gmu_w) and torch.equal(gsig, gsig_w)
