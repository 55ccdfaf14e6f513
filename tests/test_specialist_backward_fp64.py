"""The specialist TRAINING backward (csrc/cf_context.hip, wired in layers/autograd_ctx.py) against fp64 on every branch of its
kernels: the context-shifted mixture prior (cf_gmm_ctx_logprob[_tab], cf_gmm_ctx_bwd[_tab], cf_gmm_ctx_pgrad_tab), the
per-sample Conv1x1 and ActNorm (cf_conv1x1_ctx_bwd, cf_actnorm_ctx_bwd) and the small kernels of the same walk
(cf_sample_channel_sums, cf_relu_bwd, cf_add_sample_bias).  Everything goes through the C ABI; the references are plain torch
on the CPU (tests/specialist_backward_fp64_ref.py), tied to oracle/flow_oracle.py by the unmarked tests of this file.

Bars, none read off the code under test (R.bar, R.bar_mixture, R.bar_lp):
  * closed forms and autograd on well-conditioned graphs (Conv1x1, ActNorm, the sums, and the mixture gradients GIVEN the
    kernel's own log-joints): err = max|got - ref| / max(max|ref|, 1e-3) <= min(1e-4, max(2e-6, 4 x floor)), floor = the same
    reference in fp32 on the CPU;
  * mixture gradients against true fp64 autograd with the log-joints recomputed (lp = NULL): max(1e-4, 3 x floor), floor = fp32
    autograd on the same graph - with mixed responsibilities one ulp of a log-joint of size 1e4 is 1e-3 nats;
  * log-joints and log p: |delta| <= max(2e-6 max|lp|, 4 x the fp32 CPU floor).
The mixture inputs have genuinely mixed responsibilities (test_mixture_inputs_are_mixed).  Measured: profiles/specialist_backward_fp64.md."""
import ctypes
import functools
import types

import pytest
import torch

from oracle import flow_oracle as fo
from tests import specialist_backward_fp64_ref as R

DEV = "cuda:0"
SENTINEL = 12345.0

# (M, K, D, H, W, B, U keys) and the branch each is the smallest shape to reach (S, SEG: R.gmm_ctx_group, R.seg_lanes - the
# restatements of gmm_ctx_group / GmmCtxLanes in csrc/cf_context.hip):
#   (10, 8, 16, 8, 8, 37, 5)   a cifar10 level: S = 4, ragged last group (37 = 9 * 4 + 1), SEG = 64
#   (3, 4, 8, 4, 4, 600, 3)    SEG = 16, four channels per wave, two channel groups (two waves idle); three pgrad slabs of 256
#   (2, 3, 5, 7, 7, 6, 2)      H W = 49: SEG = 32, the p < HW guards; D = 5 odd with two channels per wave (dok false); N = 245:
#                              the scalar branch of stage_copy
#   (2, 2, 2, 40, 32, 5, 2)    H W = 1280 > 256: several pixel passes, the += stores of gc
#   (4, 1, 3, 1, 1, 2, 1)      H W = 1 (SEG = 1), K = 1
#   (2, 3, 33, 16, 8, 9, 2)    N = 4224: S = 2, ragged group
#   (1, 2, 65, 16, 8, 3, 2)    N = 8320: S = 1 within 64 KiB
#   (1, 2, 130, 16, 8, 2, 2)   N = 16640: S = 1 with more than 64 KiB of dynamic LDS (the raised path)
MIX = [(10, 8, 16, 8, 8, 37, 5), (3, 4, 8, 4, 4, 600, 3), (2, 3, 5, 7, 7, 6, 2), (2, 2, 2, 40, 32, 5, 2), (4, 1, 3, 1, 1, 2, 1),
       (2, 3, 33, 16, 8, 9, 2), (1, 2, 65, 16, 8, 3, 2), (1, 2, 130, 16, 8, 2, 2)]
MIX_BRANCH = {MIX[0]: (4, 64, False), MIX[1]: (4, 16, False), MIX[2]: (4, 32, False), MIX[3]: (4, 64, False), MIX[4]: (4, 1, False),
              MIX[5]: (2, 64, False), MIX[6]: (1, 64, False), MIX[7]: (1, 64, True)}        # (S, SEG, more than 64 KiB)
# seed of the draw: the first whose inputs meet the mixedness condition (three rows of responsibilities at B = 3, M = 1)
MIX_SEED = {MIX[6]: 2}
MIX_LAYOUTS = [(c, "dense") for c in MIX] + [(MIX[0], "slice"), (MIX[0], "off4"), (MIX[5], "slice"), (MIX[5], "off4")]
mid = lambda c: "-".join(map(str, c))

# (C, H W): the image levels, mnist, SMAP (C % 8 != 0: the CP padding), ATM (68 704 B of LDS: the raised path), odd everything
AFFINE = [(16, 256), (32, 64), (64, 16), (8, 256), (26, 8), (76, 72), (3, 5)]
AFFINE_CASES = [(C, HW, B, sh) for C, HW in AFFINE for sh in (True, False) for B in (1, 5)] + [(64, 16, 67, True), (64, 16, 67, False)]
# ... plus, for the ActNorm: one pixel, H W = 49 (idle lanes, a ragged 64-lane walk), C = 3 (a wave without a channel)
ACTNORM_CASES = AFFINE_CASES + [(C, HW, B, sh) for C, HW in ((6, 1), (10, 49), (3, 64)) for sh in (True, False) for B in (1, 5)]
aid = lambda c: "C%d-HW%d-B%d-%s" % (c[0], c[1], c[2], "shared" if c[3] else "alone")


@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


def _report(case, what, **kv):
    print("REPORT|%s|%s|%s" % (case, what, "|".join("%s=%s" % (k, ("%.3e" % v) if isinstance(v, float) else v) for k, v in kv.items())))


# ================================================================================================ references (CPU, computed once)
@functools.lru_cache(maxsize=None)
def _mix(case):
    """Inputs of a MIX case, its fp64 autograd run (lp, out, gx, gc) and the floors of fp32 autograd on the same graph: relative
    for gx / gc, absolute for lp / out.  Read-only."""
    c = R.mixture_case(*case, seed=MIX_SEED.get(case, 0))
    c.ref = R.mixture_autograd(c, torch.float64)
    r32 = R.mixture_autograd(c, torch.float32)
    c.floor = {k: R.rel_err(r32[k], c.ref[k]) for k in ("gx", "gc")}
    c.floor_abs = {k: (r32[k].double() - c.ref[k]).abs().max().item() for k in ("lp", "out")}
    return c


def _given_lp_refs(c, lp):
    """fp64 closed form given lp and the floor of the same closed form in fp32 (same lp)."""
    ref = R.mixture_given_lp(c, lp.double(), torch.float64)
    r32 = R.mixture_given_lp(c, lp.float(), torch.float32)
    return ref, {k: R.rel_err(r32[k], ref[k]) for k in ref}


@functools.lru_cache(maxsize=None)
def _affine(kind, C, HW, B, shared, trained):
    o = R.affine_operands(C, HW, B, seed=1000 * C + HW + B, trained=trained, with_shared=shared)
    fn = R.conv1x1_ctx_grads if kind == "conv" else R.actnorm_ctx_grads
    o.ref = fn(o, torch.float64)
    r32 = fn(o, torch.float32)
    o.floor = {k: R.rel_err(r32[k], o.ref[k]) for k in o.ref}
    return o


# ================================================================================================ CPU: the references and the inputs
@pytest.mark.parametrize("case", MIX, ids=mid)
def test_mixture_inputs_are_mixed(case):
    """Per case: the shape reaches the branch it is listed for (S, SEG, the raised LDS path, ragged groups), and the share of
    (sample, mixture) rows whose largest fp64 responsibility exceeds 0.99 is <= 0.5 (independent randn parameters give 1.0: a
    softmax of zeros and a one, which multiplies the softmax and segmented-sum parts of the kernels by 0 or 1).  K = 1 has no
    responsibilities to mix: the condition is void there.  The 3 % margin from the LDS thresholds holds for every shape but
    the two S = 1 ones, whose stated sizes are 1.7 % / 1.6 % past the S = 2 / 64 KiB limits: >= 1.5 % is asserted for those."""
    M, K, D, H, W, B, U = case
    c = _mix(case)
    S, lds = R.gmm_ctx_group(c.N, M * K)
    assert (S, R.seg_lanes(H * W), lds > 64 * 1024) == MIX_BRANCH[case]
    margin = R.threshold_margin(c.N, M * K)
    assert margin >= (0.015 if S == 1 else 0.03), margin
    if case in (MIX[0], MIX[5]):
        assert B % S != 0 and c.N % 4 == 0
    resp = torch.softmax(c.ref["lp"], -1).max(-1).values
    share = (resp > 0.99).double().mean().item()
    _report(mid(case), "inputs", S=S, lds=lds, margin=margin, share=share, median=resp.median().item(), max_lp=c.ref["lp"].abs().max().item())
    assert torch.isfinite(c.ref["lp"]).all()
    if K > 1:
        assert share <= 0.5, share


@pytest.mark.parametrize("case", MIX, ids=mid)
def test_given_lp_closed_form_equals_autograd(case):
    """The closed form given lp, with lp from the fp64 run itself, is the autograd gradient to 1e-10 (gx, gc); its batch sums are
    the autograd gradients of mG and sG."""
    c = _mix(case)
    cf = R.mixture_given_lp(c, c.ref["lp"], torch.float64)
    for k in ("gx", "gc"):
        assert R.rel_err(cf[k], c.ref[k]) <= 1e-10, (k, R.rel_err(cf[k], c.ref[k]))
    d = lambda t: t.double()
    mG, sG = d(c.mG).requires_grad_(True), d(c.sG).requires_grad_(True)
    lp = R.mixture_logjoints(d(c.x), mG, sG, torch.log_softmax(d(c.wG), -1), d(c.c))
    (torch.logsumexp(lp, -1) * d(c.g)).sum().backward()
    assert R.rel_err(cf["gmG"], mG.grad) <= 1e-10 and R.rel_err(cf["gsG"], sG.grad) <= 1e-10
    r = torch.softmax(c.ref["lp"], -1) * d(c.g).unsqueeze(-1)
    pg = R.mixture_param_grads(c, r, torch.float64)
    assert R.rel_err(pg["gmG"], mG.grad) <= 1e-10 and R.rel_err(pg["gsG"], sG.grad) <= 1e-10


def test_mixture_formula_equals_the_oracle():
    """mixture_logjoints = the formula of fo.gmm_ctx_logprob: the oracle with the shift rows as ONE embedding table and the sample
    index as the context gives the same log p and, by autograd, the same gradients of x and the shifts, to 1e-12."""
    c = _mix(MIX[2])
    d = lambda t: t.double()
    x, tab = d(c.x).requires_grad_(True), d(c.c).reshape(c.B, -1).requires_grad_(True)
    out = fo.gmm_ctx_logprob(x, d(c.mG), d(c.sG), d(c.wG), [tab], torch.arange(c.B).view(-1, 1))
    (out * d(c.g)).sum().backward()
    assert R.rel_err(c.ref["out"], out) <= 1e-12
    assert R.rel_err(c.ref["gx"], x.grad) <= 1e-12 and R.rel_err(c.ref["gc"], tab.grad.view_as(c.ref["gc"])) <= 1e-12


@pytest.mark.parametrize("shared", [True, False])
def test_affine_formulas_equal_the_oracle(shared):
    """conv1x1_ctx / actnorm_ctx = fo.conv1x1_ctx_fwd / fo.actnorm_ctx_fwd with the identity as the CN net (m = c, logp_c = 0):
    z, the log-det (up to the constant H W log|det Wm| of the oracle) and the gradients of x and m to 1e-12."""
    C, H, W, B = 5, 3, 2, 4
    o = R.affine_operands(C, H * W, B, seed=3, trained=True, with_shared=shared)
    d = lambda t: None if t is None else t.double()
    zero = torch.zeros(B, dtype=torch.float64)
    for kind in ("conv", "act"):
        x = d(o.x).view(B, C, H, W).clone().requires_grad_(True)
        if kind == "conv":
            m = d(o.m).reshape(B, C * C).clone().requires_grad_(True)
            z, ldj = fo.conv1x1_ctx_fwd(x, d(o.Wm), torch.eye(C * C, dtype=torch.float64), torch.zeros(C * C, dtype=torch.float64), m, zero, shared)
            zr, lr = R.conv1x1_ctx(d(o.x), d(o.m), d(o.Wm))
            if shared:
                lr = lr + H * W * torch.linalg.slogdet(d(o.Wm))[1]
            want = R.conv1x1_ctx_grads(o, torch.float64)
        else:
            m = d(o.ma).clone().requires_grad_(True)
            z, ldj = fo.actnorm_ctx_fwd(x, d(o.t), d(o.logs), torch.eye(2 * C, dtype=torch.float64), torch.zeros(2 * C, dtype=torch.float64), m, zero,
                                        shared)
            zr, lr = R.actnorm_ctx(d(o.x), d(o.ma), d(o.t), d(o.logs))
            want = R.actnorm_ctx_grads(o, torch.float64)
        ((z * d(o.gz).view(B, C, H, W)).sum() + (ldj * d(o.gld)).sum()).backward()
        assert R.rel_err(zr, z.flatten(2)) <= 1e-12 and R.rel_err(lr, ldj) <= 1e-12
        assert R.rel_err(want["gx"], x.grad.flatten(2)) <= 1e-12 and R.rel_err(want["gm"], m.grad.view_as(want["gm"])) <= 1e-12
        if kind == "conv":
            assert (want["gm"].triu(1) == 0).all()


# ---- the tests must be able to fail: defects restated in fp64, against the bars of the GPU tests
def _exceeds(case, what, bad, ref, bars, keys):
    for k in keys:
        err = R.rel_err(bad[k], ref[k])
        _report(case, "defect " + what, tensor=k, err=err, bar=bars[k], factor=err / bars[k])
        assert err >= 10.0 * bars[k], (case, what, k, err, bars[k])


@pytest.mark.parametrize("case", MIX, ids=mid)
def test_mixture_defects_break_the_bars(case):
    """Restated in fp64: the last sample of a ragged group dropped (gx, gc and the batch sums gmG, gsG), softplus' missing from
    gc[1] / gsG, and `=` for the `+=` of the second pixel pass (gc) each exceed every bar they reach at least 10-fold - the
    given-lp bar and the autograd bar (fp32 floors of this case)."""
    M, K, D, H, W, B, U = case
    c = _mix(case)
    lp = c.ref["lp"]
    ref, floor = _given_lp_refs(c, lp)
    # the larger of the two bars a tensor is held to (gmG / gsG: the closed form given r; the host wiring test holds them to the autograd rule)
    bars = {k: max(R.bar(floor[k]), R.bar_mixture(c.floor.get(k, floor[k]))) for k in ref}
    S = MIX_BRANCH[case][0]
    if B % S != 0:
        _exceeds(mid(case), "drop_last", R.mixture_given_lp(c, lp, torch.float64, "drop_last", S), ref, bars, ("gx", "gc", "gmG", "gsG"))
    bad = R.mixture_given_lp(c, lp, torch.float64, "no_dsig")
    assert torch.equal(bad["gx"], ref["gx"]) and torch.equal(bad["gc"][:, 0], ref["gc"][:, 0])
    _exceeds(mid(case), "no_dsig", {"gc": bad["gc"], "gsG": bad["gsG"]}, ref, bars, ("gc", "gsG"))
    if H * W > 4 * R.seg_lanes(H * W):
        _exceeds(mid(case), "second_pass", R.mixture_given_lp(c, lp, torch.float64, "second_pass"), ref, bars, ("gc",))


@pytest.mark.parametrize("case,slab", [(MIX[1], 256), (MIX[1], 7), (MIX[5], 7), (MIX[5], 1)], ids=lambda v: mid(v) if isinstance(v, tuple) else str(v))
def test_omitted_slab_breaks_the_bars(case, slab):
    """One slab's partial left out of the sum (the last, ragged one, and the first) exceeds the bars of gmG and gsG 10-fold."""
    c = _mix(case)
    r = torch.softmax(c.ref["lp"], -1) * c.g.double().unsqueeze(-1)
    ref = R.mixture_param_grads(c, r, torch.float64)
    f32 = R.mixture_param_grads(c, r, torch.float32)
    bars = {k: R.bar(R.rel_err(f32[k], ref[k])) for k in ref}
    nb = (c.B + slab - 1) // slab
    for omit in (nb - 1, 0):
        _exceeds(mid(case), "omit_slab %d of %d" % (omit, nb), R.mixture_param_grads(c, r, torch.float64, slab, omit), ref, bars, ("gmG", "gsG"))


@pytest.mark.parametrize("case", AFFINE_CASES, ids=aid)
@pytest.mark.parametrize("trained", [False, True])
def test_conv1x1_defects_break_the_bars(case, trained):
    """H W gld missing from the diagonal of gm, and the diagonal of W_b^T taken from m instead of exp(m) in gx, exceed their bars
    10-fold."""
    o = _affine("conv", *case, trained)
    bars = {k: R.bar(o.floor[k]) for k in o.ref}
    _exceeds(aid(case), "no_gld", R.conv1x1_ctx_grads(o, torch.float64, "no_gld"), o.ref, bars, ("gm",))
    _exceeds(aid(case), "diag_m", R.conv1x1_ctx_grads(o, torch.float64, "diag_m"), o.ref, bars, ("gx",))


# ================================================================================================ GPU helpers
def _guarded(*shape, rows=4):
    """A NaN-filled fp32 tensor of `shape` with `rows` more rows of SENTINEL behind it (the rows the missing samples of a ragged
    group would own).  Returns (tensor, check): check() asserts the sentinels are untouched."""
    n = 1
    for s in shape:
        n *= s
    extra = max(rows * (n // max(shape[0], 1)), 64)
    buf = torch.full((n + extra,), float("nan"), device=DEV)
    buf[n:] = SENTINEL
    return buf[:n].view(*shape), lambda: bool((buf[n:] == SENTINEL).all())


def _place(t, layout, Cw=None, front=False):
    """t (B, C, ...) fp32 on the device as `layout`: "dense"; "slice" = the first (front=True: the last) C channels of a tensor with
    Cw (default 2 C) channels, seeded filler in the others (a read through the wrong stride finds other numbers, not zeros);
    "off4" = dense, starting 4 bytes past a 16-byte boundary.  Returns (tensor, batch stride in floats)."""
    B, inner = t.shape[0], t[0].numel()
    if layout == "dense":
        out = t.to(DEV).contiguous()
    elif layout == "slice":
        Cw = Cw or 2 * t.shape[1]
        big = torch.empty(B, Cw, *t.shape[2:], device=DEV).normal_(generator=torch.Generator(device=DEV).manual_seed(B + Cw))
        out = big[:, Cw - t.shape[1]:] if front else big[:, :t.shape[1]]
        out.copy_(t)
        assert out.stride(0) == Cw * (inner // t.shape[1]) > inner
    else:
        flat = torch.empty(B * inner + 4, device=DEV).normal_(generator=torch.Generator(device=DEV).manual_seed(B))
        assert flat.data_ptr() % 16 == 0
        out = flat[1:1 + B * inner].view(t.shape)
        out.copy_(t)
        assert out.data_ptr() % 16 == 4
    return out, out.stride(0)


def _mix_device(c):
    """Parameters of a mixture case on the device and the tables of the table form (cf_gmm_ctx_tables)."""
    from contextflow_amd.layers import _hip
    dv = lambda t: t.contiguous().to(DEV)
    MK, HW = c.M * c.K, c.H * c.W
    d = types.SimpleNamespace(mG=dv(c.mG), sG=dv(c.sG), logw=dv(c.logw), c=dv(c.c), g=dv(c.g), key=dv(c.key.to(torch.int32)))
    d.inv, d.dsig = torch.empty(c.U, MK * c.N, device=DEV), torch.empty(c.U, MK * c.N, device=DEV)
    d.lsum = torch.empty(c.U, MK, device=DEV)
    _hip.call("cf_gmm_ctx_tables", _hip.p(d.sG), _hip.p(dv(c.cs_tab)), _hip.p(d.inv), _hip.p(d.dsig), _hip.p(d.lsum), c.U, MK, c.D, HW,
              _hip.stream())
    return d


def _mix_forward(c, d, x, xbs, tab, out, lp, accumulate):
    from contextflow_amd.layers import _hip
    p, dims = _hip.p, (c.B, c.M, c.K, c.D, c.H * c.W, xbs, accumulate, _hip.stream())
    if tab:
        _hip.call("cf_gmm_ctx_logprob_tab", p(x), p(d.mG), p(d.inv), p(d.lsum), p(d.logw), p(d.c), None, p(d.key), p(out), p(lp), *dims)
    else:
        _hip.call("cf_gmm_ctx_logprob", p(x), p(d.mG), p(d.sG), p(d.logw), p(d.c), p(out), p(lp), *dims)


def _mix_backward(c, d, x, xbs, tab, lp, gx, gc):
    from contextflow_amd.layers import _hip
    p, dims = _hip.p, (c.B, c.M, c.K, c.D, c.H * c.W, xbs, _hip.stream())
    if tab:
        _hip.call("cf_gmm_ctx_bwd_tab", p(x), p(d.mG), p(d.inv), p(d.dsig), p(d.lsum), p(d.logw), p(d.c), p(d.key), p(d.g), p(lp), p(gx), p(gc),
                  *dims)
    else:
        _hip.call("cf_gmm_ctx_bwd", p(x), p(d.mG), p(d.sG), p(d.logw), p(d.c), p(d.g), p(lp), p(gx), p(gc), *dims)


class _Fails(list):
    def hold(self, case, what, key, got, ref, floor, tol):
        assert torch.isfinite(got).all(), (case, what, key)
        err = R.rel_err(got, ref)
        _report(case, what, tensor=key, err=err, floor=floor, bar=tol, ratio=err / tol)
        if not err <= tol:
            self.append("%s %s: err %.3e > bar %.3e (floor %.3e)" % (what, key, err, tol, floor))

    def hold_abs(self, case, what, key, got, ref, floor_abs):
        assert torch.isfinite(got).all(), (case, what, key)
        err, tol = (got.detach().cpu().double().reshape(ref.shape) - ref).abs().max().item(), R.bar_lp(ref, floor_abs)
        _report(case, what, tensor=key, err=err, floor=floor_abs, bar=tol, ratio=err / tol)
        if not err <= tol:
            self.append("%s %s: |delta| %.3e > bar %.3e (floor %.3e)" % (what, key, err, tol, floor_abs))


# ================================================================================================ GPU: the mixture
@pytest.mark.gpu
@pytest.mark.parametrize("case,layout", MIX_LAYOUTS, ids=lambda v: mid(v) if isinstance(v, tuple) else v)
def test_mixture_kernels_against_fp64(L, case, layout):
    """Both forms (direct: the scale shifts through softplus in the kernel; table: cf_gmm_ctx_tables and a key per sample) on the
    same inputs.  Forward with accumulate = 1 on a pre-filled out, the kept log-joints; the backward with the kept lp against the
    closed form given that lp, and with lp = NULL against true autograd.  Every output starts as NaN with sentinel rows behind it:
    an element no thread wrote stays NaN, a row written for a missing sample of the ragged last group breaks a sentinel.  layout:
    x as the first D channels of a wider tensor (x_bstride > N), x 4 bytes off 16-byte alignment with N % 4 = 0 (stage_copy's
    scalar branch on a vectorisable size).  B = 0 returns 0 from every entry."""
    from contextflow_amd.layers import _hip
    M, K, D, H, W, B, U = case
    c, tag = _mix(case), mid(case) + "/" + layout
    d = _mix_device(c)
    x, xbs = _place(c.x, layout)
    assert (layout == "dense") == (xbs == c.N and x.data_ptr() % 16 == 0)
    fails = _Fails()
    gen = torch.Generator().manual_seed(B)
    for tab in (False, True):
        form = "table" if tab else "direct"
        pre = torch.randn(B, M, generator=gen)
        out, out_ok = _guarded(B, M)
        out.copy_(pre)
        lp, lp_ok = _guarded(B, M * K)
        _mix_forward(c, d, x, xbs, tab, out, lp, 1)
        torch.cuda.synchronize()
        assert out_ok() and lp_ok(), (tag, form, "forward wrote behind its outputs")
        fails.hold_abs(tag, form, "out", out.cpu().double() - pre.double(), c.ref["out"], c.floor_abs["out"])
        fails.hold_abs(tag, form, "lp", lp, c.ref["lp"], c.floor_abs["lp"])
        out2, _ = _guarded(B, M)
        _mix_forward(c, d, x, xbs, tab, out2, None, 0)                      # accumulate = 0 overwrites (NaN underneath), no lp_out
        fails.hold_abs(tag, form, "out(store)", out2, c.ref["out"], c.floor_abs["out"])
        # backward with the kept log-joints: the arithmetic behind the responsibilities
        ref_lp, floor_lp = _given_lp_refs(c, lp.cpu().view(B, M, K))
        gx, gx_ok = _guarded(B, D, H, W)
        gc, gc_ok = _guarded(B, 2 * M * K * D)
        _mix_backward(c, d, x, xbs, tab, lp, gx, gc)
        torch.cuda.synchronize()
        assert gx_ok() and gc_ok(), (tag, form, "backward wrote behind its outputs")
        for k, got in (("gx", gx), ("gc", gc)):
            fails.hold(tag, form + " given lp", k, got, ref_lp[k], floor_lp[k], R.bar(floor_lp[k]))
        # ... and with the log-joints recomputed, against true autograd
        gx, gx_ok = _guarded(B, D, H, W)
        gc, gc_ok = _guarded(B, 2 * M * K * D)
        _mix_backward(c, d, x, xbs, tab, None, gx, gc)
        torch.cuda.synchronize()
        assert gx_ok() and gc_ok(), (tag, form, "backward (lp = NULL) wrote behind its outputs")
        for k, got in (("gx", gx), ("gc", gc)):
            fails.hold(tag, form + " lp=NULL", k, got, c.ref[k], c.floor[k], R.bar_mixture(c.floor[k]))
    lib, N_ = _hip.lib(), None
    assert lib.cf_gmm_ctx_logprob(*[N_] * 7, 0, M, K, D, H * W, c.N, 1, N_) == 0
    assert lib.cf_gmm_ctx_logprob_tab(*[N_] * 10, 0, M, K, D, H * W, c.N, 1, N_) == 0
    assert lib.cf_gmm_ctx_bwd(*[N_] * 9, 0, M, K, D, H * W, c.N, N_) == 0
    assert lib.cf_gmm_ctx_bwd_tab(*[N_] * 12, 0, M, K, D, H * W, c.N, N_) == 0
    assert lib.cf_gmm_ctx_pgrad_tab(*[N_] * 9, 0, M, K, D, H * W, c.N, 256, N_) == 0
    assert not fails, (tag, fails)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [MIX[1], MIX[5]], ids=mid)
def test_mixture_parameter_gradient_slabs(L, case):
    """cf_gmm_ctx_pgrad_tab with r as gmm_ctx_backward forms it (softmax of the kept log-joints times the upstream gradient, on the
    device) and slab = 256 (three slabs at B = 600, the last ragged), 7, 1, B and B + 5: the per-slab partials, summed in fp64,
    against the closed form given the same r.  The slab = 7 run reads a batch-strided x.  Partials start as NaN with a sentinel slab
    behind them."""
    from contextflow_amd.layers import _hip
    M, K, D, H, W, B, U = case
    c = _mix(case)
    d = _mix_device(c)
    p, st = _hip.p, _hip.stream()
    x, xbs = _place(c.x, "dense")
    out, lp = torch.empty(B, M, device=DEV), torch.empty(B, M * K, device=DEV)
    _mix_forward(c, d, x, xbs, True, out, lp, 0)
    r = (torch.softmax(lp.view(B, M, K), dim=-1) * d.g.unsqueeze(-1)).reshape(B, M * K).contiguous()
    ref = R.mixture_param_grads(c, r.cpu(), torch.float64)
    f32 = R.mixture_param_grads(c, r.cpu(), torch.float32)
    floor = {k: R.rel_err(f32[k], ref[k]) for k in ref}
    fails = _Fails()
    for slab in (256, 7, 1, B, B + 5):
        nb = (B + slab - 1) // slab
        xs, xs_bs = _place(c.x, "slice" if slab == 7 else "dense")
        pgm, m_ok = _guarded(nb, M * K, c.N, rows=1)
        pgs, s_ok = _guarded(nb, M * K, c.N, rows=1)
        _hip.call("cf_gmm_ctx_pgrad_tab", p(xs), p(d.mG), p(d.inv), p(d.dsig), p(d.c), p(d.key), p(r), p(pgm), p(pgs), B, M, K, D, H * W, xs_bs,
                  slab, st)
        torch.cuda.synchronize()
        assert m_ok() and s_ok(), (slab, "wrote behind the partials")
        for k, got in (("gmG", pgm), ("gsG", pgs)):
            assert torch.isfinite(got).all(), (slab, k)
            fails.hold(mid(case), "pgrad slab=%d" % slab, k, got.double().sum(0), ref[k], floor[k], R.bar(floor[k]))
    assert not fails, fails


@pytest.mark.gpu
def test_mixture_host_wiring_against_fp64(L):
    """A GaussianMixtureDistribution with an embedding context net and contextflow = False, as create_model builds a specialist
    prior, size (8, 4, 4), B = 600: _log_prob_ctx with a tape, then autograd_ctx.gmm_ctx_backward.  log p, gx and the gradients
    of mG, sG, wG and both embedding tables against fp64 autograd through fo.gmm_ctx_logprob at max(1e-4, 3 x floor), floor =
    fp32 autograd through the same function."""
    from contextflow_amd.layers import autograd_ctx
    M, K, D, H, W, B, U, Um = 3, 4, 8, 4, 4, 600, 3, 2
    c = R.mixture_case(M, K, D, H, W, B, U, seed=1, Um=Um)
    cn = L.ContextEncoder([Um, U], "embed", "eyesample", (2 * M * K * D // 2,), init="zeros")
    dist = L.GaussianMixtureDistribution(size=(D, H, W), mixtures=M, components=K, context_net=cn, contextflow=False).to(DEV)
    embs = list(dist.context_net[0]._embeddings)
    with torch.no_grad():
        dist.mG.copy_(c.mG); dist.sG.copy_(c.sG); dist.wG.copy_(c.wG)
        embs[0].weight.copy_(c.cm_tab); embs[1].weight.copy_(c.cs_tab.reshape(U, -1))
    assert all(p.requires_grad for p in (dist.mG, dist.sG, dist.wG))
    context = torch.stack([c.ckey, c.key], 1)

    def run(dtype):
        leaves = [t.to(dtype).clone().requires_grad_(True) for t in (c.x, c.mG, c.sG, c.wG, c.cm_tab, c.cs_tab.reshape(U, -1))]
        x, mG, sG, wG, e0, e1 = leaves
        outs = []
        for b0 in range(0, B, 64):
            o = fo.gmm_ctx_logprob(x[b0:b0 + 64], mG, sG, wG, [e0, e1], context[b0:b0 + 64], chunk=64)
            (o * c.g[b0:b0 + 64].to(dtype)).sum().backward()
            outs.append(o.detach())
        return dict(zip(("gx", "mG", "sG", "wG", "emb0", "emb1"), (t.grad for t in leaves))), torch.cat(outs, 0)
    ref, out_ref = run(torch.float64)
    f32, out_32 = run(torch.float32)
    tape, grads = [], {}
    out = dist._log_prob_ctx(c.x.to(DEV), context.to(DEV), tape)
    assert len(tape) == 1 and tape[0].tab is not None and tape[0].lp is not None
    gx = autograd_ctx.gmm_ctx_backward(tape[0], c.g.to(DEV), grads)
    torch.cuda.synchronize()
    got = {"gx": gx, "mG": grads[dist.mG], "sG": grads[dist.sG], "wG": grads[dist.wG], "emb0": grads[embs[0].weight], "emb1": grads[embs[1].weight]}
    fails = _Fails()
    fails.hold_abs("host", "wiring", "out", out, out_ref, (out_32.double() - out_ref).abs().max().item())
    for k, t in got.items():
        floor = R.rel_err(f32[k], ref[k])
        fails.hold("host", "wiring", k, t, ref[k], floor, R.bar_mixture(floor))
    assert not fails, fails


@pytest.mark.gpu
def test_mixture_refuses_what_no_cu_holds(L):
    """M = K = D = 1, H W = 41 000: one sample needs 164 020 B of LDS, more than the 160 KiB of a CU.  Every entry point that
    launches through gmm_ctx_launch returns the unsupported code before any launch (dummy non-NULL pointers) and names the need."""
    from contextflow_amd.layers import _hip
    lib, q, N_ = _hip.lib(), ctypes.c_void_p(16), None
    HW = 41000
    assert R.gmm_ctx_group(HW, 1) == (0, 164020)
    calls = {"cf_gmm_ctx_logprob": lambda: lib.cf_gmm_ctx_logprob(*[q] * 7, 1, 1, 1, 1, HW, HW, 0, N_),
             "cf_gmm_ctx_logprob_tab": lambda: lib.cf_gmm_ctx_logprob_tab(*[q] * 10, 1, 1, 1, 1, HW, HW, 0, N_),
             "cf_gmm_ctx_bwd": lambda: lib.cf_gmm_ctx_bwd(*[q] * 9, 1, 1, 1, 1, HW, HW, N_),
             "cf_gmm_ctx_bwd_tab": lambda: lib.cf_gmm_ctx_bwd_tab(*[q] * 12, 1, 1, 1, 1, HW, HW, N_),
             "cf_gmm_ctx_bwd_data": lambda: lib.cf_gmm_ctx_bwd_data(*[q] * 11, 1, 1, 1, 1, HW, HW, N_)}
    for name, fn in calls.items():
        assert fn() == -2, name
        err = lib.cf_last_error()
        assert name.encode() in err and b"164020" in err and b"LDS" in err, (name, err)


# ================================================================================================ GPU: Conv1x1 / ActNorm with a context net
# the operand sets of every case: (values, layout of x and gz)
AFFINE_SETS = [(False, "dense"), (True, "slice"), (False, "off4")]


def _affine_run(kind, case, fails):
    from contextflow_amd.layers import _hip
    C, HW, B, shared = case
    p, st, dv = _hip.p, _hip.stream(), (lambda t: None if t is None else t.contiguous().to(DEV))
    for trained, layout in AFFINE_SETS:
        o = _affine(kind, C, HW, B, shared, trained)
        x, xbs = _place(o.x, layout)
        gz, gzbs = _place(o.gz, layout, Cw=2 * C + 3, front=True)
        if layout == "slice":
            assert xbs > C * HW and gzbs > C * HW and xbs != gzbs
        gx, gx_ok = _guarded(B, C, HW)
        if kind == "conv":
            gm, gm_ok = _guarded(B, C * C)
            _hip.call("cf_conv1x1_ctx_bwd", p(x), p(dv(o.m)), p(dv(o.Wm)), p(gz), p(dv(o.gld)), p(gx), p(gm), B, C, HW, xbs, gzbs, st)
        else:
            gm, gm_ok = _guarded(B, 2 * C)
            _hip.call("cf_actnorm_ctx_bwd", p(x), p(dv(o.ma)), p(dv(o.t)), p(dv(o.logs)), p(gz), p(dv(o.gld)), p(gx), p(gm), B, C, HW, xbs, gzbs,
                      st)
        torch.cuda.synchronize()
        what = "%s %s/%s" % (kind, "trained" if trained else "randn", layout)
        assert gx_ok() and gm_ok(), (what, "wrote behind its outputs")
        for k, got in (("gx", gx), ("gm", gm)):
            fails.hold(aid(case), what, k, got, o.ref[k], o.floor[k], R.bar(o.floor[k]))
        if kind == "conv":                                    # the exact zeros above the diagonal
            assert (gm.view(B, C, C).triu(1) == 0).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("case", AFFINE_CASES, ids=aid)
def test_conv1x1_ctx_bwd_against_fp64(L, case):
    """cf_conv1x1_ctx_bwd: gx and all of gm (the exact zeros above the diagonal included) against fp64 autograd through the
    formula of fo.conv1x1_ctx_fwd with m as a leaf, gld != 0, with Wm and with NULL.  Three operand sets per case: m = 0.3
    randn, dense; a trained-like m (diagonal in +-3, strictly-lower entries up to 1) with x and gz as channel slices of wider
    tensors (two different batch strides > C H W, as behind a SplitPrior); x and gz 4 bytes off 16-byte alignment."""
    fails = _Fails()
    _affine_run("conv", case, fails)
    assert not fails, (aid(case), fails)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ACTNORM_CASES, ids=aid)
def test_actnorm_ctx_bwd_against_fp64(L, case):
    """cf_actnorm_ctx_bwd, its first direct test: gx and both halves of gm = [d/d t_b | d/d l_b] against fp64 autograd through the
    formula of fo.actnorm_ctx_fwd, t / logs given and both NULL.  The second half is gld[b] - sum g z, a cancelling sum: the error
    is scaled by max|ref| of the whole tensor.  Operand sets as for the Conv1x1."""
    fails = _Fails()
    _affine_run("act", case, fails)
    assert not fails, (aid(case), fails)


@pytest.mark.gpu
def test_conv1x1_ctx_bwd_refuses_what_no_cu_holds(L):
    """C = 128, H W = 256 needs 328 704 B of LDS: refused on the host, no launch (dummy non-NULL pointers)."""
    from contextflow_amd.layers import _hip
    lib, q = _hip.lib(), ctypes.c_void_p(16)
    assert lib.cf_conv1x1_ctx_bwd(*[q] * 7, 1, 128, 256, 128 * 256, 128 * 256, None) == -2
    err = lib.cf_last_error()
    assert b"cf_conv1x1_ctx_bwd" in err and b"328704" in err and b"LDS" in err, err


# ================================================================================================ GPU: the small kernels of the walk
@pytest.mark.gpu
@pytest.mark.parametrize("B,C,HW", [(3, 7, 1), (5, 3, 72), (3, 5, 256), (67, 26, 72)])
def test_sample_channel_sums_against_fp64(L, B, C, HW):
    """cf_sample_channel_sums against fp64 row sums; B C is no multiple of the 4 rows of a workgroup."""
    from contextflow_amd.layers import _hip
    assert (B * C) % 4 != 0
    a = torch.randn(B, C, HW, generator=torch.Generator().manual_seed(B + HW)) + 0.5
    ref = a.double().sum(-1)
    floor = R.rel_err(a.sum(-1), ref)
    out, ok = _guarded(B, C)
    _hip.call("cf_sample_channel_sums", _hip.p(a.to(DEV)), _hip.p(out), B, C, HW, _hip.stream())
    torch.cuda.synchronize()
    fails = _Fails()
    fails.hold("B%d-C%d-HW%d" % (B, C, HW), "channel_sums", "out", out, ref, floor, R.bar(floor))
    assert ok() and not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 16384 * 256 + 77])
def test_relu_bwd_is_exact(L, n):
    """cf_relu_bwd = gy where x > 0, else +0, bit for bit: x = 0, -0.0, the denormals of both signs and the smallest normals among
    random values; n = 16384 * 256 + 77 is past one pass of the grid (the grid-stride wrap)."""
    from contextflow_amd.layers import _hip
    gen = torch.Generator().manual_seed(n)
    x, gy = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.1754944e-38, -1.1754944e-38])
    if n < 8:
        x[:] = special[:n]
    else:                                                     # at both ends and across the end of the first pass of the grid
        for at in (0, 16384 * 256 - 4, n - 8):
            x[at:at + 8] = special
    want = torch.where(x > 0, gy, torch.zeros_like(gy))
    out, ok = _guarded(n, rows=64)
    _hip.call("cf_relu_bwd", _hip.p(x.to(DEV)), _hip.p(gy.to(DEV)), _hip.p(out), n, _hip.stream())
    torch.cuda.synchronize()
    assert ok()
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,HW", [(3, 5, 7), (2, 26, 49), (5, 4, 64)])
@pytest.mark.parametrize("relu", [0, 1])
def test_add_sample_bias_rounds_once(L, B, C, HW, relu):
    """cf_add_sample_bias: h + bias[b, c] (then ReLU) equals the fp64 sum rounded once to fp32, bit for bit; H W = 7 and 49 are no
    multiples of 4."""
    from contextflow_amd.layers import _hip
    gen = torch.Generator().manual_seed(B * C + HW)
    h, bias = torch.randn(B, C, HW, generator=gen), torch.randn(B, C, generator=gen)
    want = h.double() + bias.double().unsqueeze(-1)
    if relu:
        want = want.clamp_min(0.0)
    buf, ok = _guarded(B, C, HW)
    buf.copy_(h)
    _hip.call("cf_add_sample_bias", _hip.p(buf), _hip.p(bias.to(DEV)), B, C, HW, relu, _hip.stream())
    torch.cuda.synchronize()
    assert ok()
    assert torch.equal(buf.cpu(), want.float())
