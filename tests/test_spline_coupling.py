"""SplineCoupling: the rational-quadratic spline with the knots of every element read from a conditioner - kernels
(cf_spline_coupling, cf_spline_coupling_bwd), layer, training backward, score, sampling direction.

References: tests/spline_coupling_ref.py in fp64 (pinned here to the reference implementation's recorded values,
tests/golden/unit_spline_coupling.npz); every floor is the same restatement run in fp32 on the CPU.

Bars.  Forward / inverse quantities (z, x, ldj) are in units of max(1, max|ref|), the bar max(2e-6, 4 x floor): 2e-6 is a few
fp32 roundings of an O(1) value, the floor carries the conditioning of the case (a bin of the minimum width 2e-3 tail_bound
turns an input rounding of 6e-8 |x| into 1e-5 of theta).  For a composed quantity (the round trip, the inverse's log-det
against the forward's at the recovered input) the floor is the fp32 restatement's error of that same composition.
Backward quantities (gx, gh) are in units of the largest entry of the reference, the bar min(1e-4, max(2e-6, 4 x the error of
fp32 autograd through the restatement)): the rule of tests/test_decode_grad.py."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import flow_oracle as fo
from tests import spline_coupling_ref as ref
from tests.helpers import bpd

DEV = "cuda:0"
BPD_TOL = 1e-5
TB = 3.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unit_spline_coupling.npz")

# (B, C, H, W, K): less than one wave per sample; more elements than one pass of a workgroup; odd half and W = 1; smallest K and
# sizes that are no multiple of 4; largest K
SHAPES = [(3, 4, 2, 2, 5), (2, 8, 16, 16, 8), (1, 26, 8, 1, 5), (5, 6, 3, 5, 2), (2, 64, 4, 4, 16)]
SLICE_SHAPE = (4, 16, 16, 16, 8)          # given as the channel or the batch slice of a larger tensor
ALL_SHAPES = SHAPES + [SLICE_SHAPE]


@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


def _rel(got, want, unit_floor=1.0):
    want = want.double()
    return (got.double().cpu() - want).abs().max().item() / max(unit_floor, want.abs().max().item())


def _bar(floor):
    return max(2e-6, 4.0 * floor)


# ------------------------------------------------------------------------------------------ inputs and references (CPU, once)
@functools.lru_cache(maxsize=None)
def fwd_case(shape):
    """h ~ 1.5 randn (uneven bins); x1 ~ 2 randn scaled so that about a tenth lies outside the tails; points exactly on
    +-tail_bound and on (the fp32 values nearest to) fp64 knots of the widths - as inputs of the inverse the same values sit on
    or next to nothing special, so the inverse gets its own points on the knots of the heights.  Returns the fp32 inputs, the
    fp64 results and the fp32 floors of forward, inverse, round trip and the inverse's log-det."""
    B, C, H, W, K = shape
    D = C // 2
    g = torch.Generator().manual_seed(sum(shape) * 7 + K)
    h = 1.5 * torch.randn(B, D * (3 * K - 1), H, W, generator=g)
    x = torch.randn(B, C, H, W, generator=g)
    x1 = 2.0 * torch.randn(B, D, H, W, generator=g)
    x1 = x1 * (TB / x1.abs().flatten().quantile(0.9))
    zi1 = x1.flip(0).flip(1).clone()
    cw, ch, _ = ref.knots(ref.split_params(h.double(), D, K), K, TB)
    f1, fz = x1.view(-1), zi1.view(-1)
    n = f1.numel()
    f1[0], f1[1 % n] = TB, -TB
    fz[0], fz[1 % n] = -TB, TB
    for i in range(2, min(n, 10)):
        k = 1 + i % (K - 1)
        f1[i] = cw.reshape(n, K + 1)[i, k].float()
        fz[i] = ch.reshape(n, K + 1)[i, k].float()
    x[:, D:] = x1
    zi = x.clone()
    zi[:, D:] = zi1
    out = dict(x=x, h=h, zi=zi)
    for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        xd, hd, zd = x.to(dt), h.to(dt), zi.to(dt)
        z, ldj = ref.coupling_map(xd, hd, K, TB)
        xi, ldji = ref.coupling_map(zd, hd, K, TB, inverse=True)
        xrt, ldj_rt = ref.coupling_map(z, hd, K, TB, inverse=True)          # round trip, and the inverse's log-det at its output
        ldj_at = ref.coupling_map(xi, hd, K, TB)[1]                          # the forward's log-det at the recovered input
        out.update({"z" + tag: z, "ldj" + tag: ldj, "xi" + tag: xi, "ldji" + tag: ldji, "xrt" + tag: xrt,
                    "ldjgap" + tag: ldji - ldj_at})
    fl = lambda a: _rel(out[a + "32"], out[a + "64"])
    # (the gap between the inverse's log-det and the forward's at the recovered input is 0 in exact arithmetic: its floor is the gap
    # the fp32 restatement leaves, in units of the log-det)
    out["floor"] = dict(z=fl("z"), ldj=fl("ldj"), xi=fl("xi"), ldji=fl("ldji"), xrt=_rel(out["xrt32"], x),
                        ldjgap=out["ldjgap32"].abs().max().item() / max(1.0, out["ldj64"].abs().max().item()))
    return out


@functools.lru_cache(maxsize=None)
def bwd_case(shape):
    """Nothing sits on a discontinuity of the parameter gradient: per element a bin and a position theta in [0.05, 0.95] are
    drawn and x1 is placed there from the fp64 knots; a tenth of the elements lie outside the tails, at least 1e-3 tail_bound
    from the bound.  Returns inputs, the fp64 autograd gradients and the fp32 autograd floors."""
    B, C, H, W, K = shape
    D = C // 2
    g = torch.Generator().manual_seed(sum(shape) * 11 + K)
    h = 1.5 * torch.randn(B, D * (3 * K - 1), H, W, generator=g)
    x = torch.randn(B, C, H, W, generator=g)
    cw, _, _ = ref.knots(ref.split_params(h.double(), D, K), K, TB)
    k = torch.randint(0, K, (B, D, H, W, 1), generator=g)
    th = 0.05 + 0.9 * torch.rand(B, D, H, W, generator=g, dtype=torch.float64)
    lo, hi = cw.gather(-1, k)[..., 0], cw.gather(-1, k + 1)[..., 0]
    x1 = lo + th * (hi - lo)
    out_mask = torch.rand(B, D, H, W, generator=g) < 0.1
    sign = torch.where(torch.rand(B, D, H, W, generator=g) < 0.5, -1.0, 1.0).double()
    far = sign * TB * (1.0 + 2e-3 + 0.5 * torch.rand(B, D, H, W, generator=g, dtype=torch.float64))
    x1 = torch.where(out_mask, far, x1).float()
    x[:, D:] = x1
    gz = torch.randn(B, C, H, W, generator=g)
    gld = torch.randn(B, generator=g)
    out = dict(x=x, h=h, gz=gz, gld=gld, k=k[..., 0], outside=out_mask)
    for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        xd, hd = x.to(dt).clone().requires_grad_(True), h.to(dt).clone().requires_grad_(True)
        z, ldj = ref.coupling_map(xd, hd, K, TB)
        ((z * gz.to(dt)).sum() + (ldj * gld.to(dt)).sum()).backward()
        out["gx" + tag], out["gh" + tag] = xd.grad, hd.grad
    scale = lambda a: out[a + "64"].abs().max().item()
    out["floor"] = dict(gx=(out["gx32"].double() - out["gx64"]).abs().max().item() / scale("gx"),
                        gh=(out["gh32"].double() - out["gh64"]).abs().max().item() / scale("gh"))
    return out


def _apply(x, h, K, inverse, ldj=True):
    """cf_spline_coupling through the C ABI on device tensors; x may be a strided view."""
    from contextflow_amd.layers.coupling import spline_coupling_apply
    return spline_coupling_apply(x, h, K, TB, inverse, inverse_ldj=ldj)


# ------------------------------------------------------------------------------------------ CPU
def test_restatement_equals_the_recorded_reference_values():
    """The fp64 restatement against `unconstrained_rational_quadratic_spline` of the reference implementation (recorded by
    tests/golden/make_golden_spline_coupling.py), forward and inverse, to 1e-12; K in {2, 5, 8, 16}; points outside the tails, on
    +-tail_bound and on knots are in the fixture."""
    fx = np.load(GOLDEN)
    tb = float(fx["tail_bound"])
    assert sorted(int(k) for k in fx["cases"]) == [2, 5, 8, 16]
    for K in (int(k) for k in fx["cases"]):
        t = lambda n: torch.from_numpy(fx["K%d_%s" % (K, n)])
        p = torch.cat([t("uw"), t("uh"), t("ud")], -1)
        assert p.shape == (t("x").numel(), 3 * K - 1) and p.dtype == torch.float64
        assert (t("x").abs() > tb).any() and (t("x") == tb).any() and (t("x") == -tb).any()
        z, lad = ref.rqs(t("x"), p, K, tb)
        xi, ladi = ref.rqs(t("zi"), p, K, tb, inverse=True)
        for got, want in ((z, t("z")), (lad, t("lad")), (xi, t("xi")), (ladi, -t("ladi"))):      # (the reference returns -lad for the inverse)
            assert (got - want).abs().max().item() <= 1e-12, K


def test_construction_errors_and_state_dict_keys():
    import contextflow_amd as cfa
    S = cfa.layers.SplineCoupling
    for bad in (dict(data_channels=5), dict(data_channels=4, bins=1), dict(data_channels=4, bins=17)):
        with pytest.raises(ValueError):
            S(**bad)
    with pytest.raises(TypeError):
        S(4, context_net=object())
    m = S(6, kernel_size=(3, 3), padding=(1, 1), bins=5)
    assert list(m.state_dict().keys()) == ["NN.%d.%s" % (i, n) for i in (0, 2, 4) for n in ("weight", "bias")]
    assert list(m.state_dict().keys()) == list(cfa.layers.Coupling(6, (3, 3), (1, 1)).state_dict().keys())
    assert tuple(m.NN[4].weight.shape) == (3 * (3 * 5 - 1), 12, 1, 1) and tuple(m.NN[2].weight.shape) == (12, 12, 3, 3)
    assert not m.NN[4].weight.any() and not m.NN[4].bias.any()
    assert m.NN[2].padding_mode == "reflect"


@pytest.mark.parametrize("name", ["mnist", "cifar10", "smap"])
def test_create_model_builds_spline_flows(name):
    import contextflow_amd as cfa
    cfg, data_size, M = cfa.preset_config(name, coupling="spline")
    model = cfa.create_model(cfg, data_size, M)
    base = cfa.create_model(*cfa.preset_config(name, coupling="conv"))
    kinds = [type(m).__name__ for m in model.sequence_modules]
    assert kinds == [("SplineCoupling" if type(m).__name__ == "Coupling" else type(m).__name__) for m in base.sequence_modules]
    assert kinds.count("SplineCoupling") == cfg["num_blocks"] * cfg["block_size"]
    krn = (3, 1) if name == "smap" else (3, 3)
    assert all(tuple(m.NN[2].kernel_size) == krn for m in model.sequence_modules if type(m).__name__ == "SplineCoupling")
    with pytest.raises(NotImplementedError):
        cfa.create_model(dict(cfg, generalist=False), data_size, M, contexts=(4,))


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_fp32_restatement_picks_the_fp64_bin(shape):
    """Condition of the backward comparison: no element is excluded, so none may sit where fp32 and fp64 choose different bins."""
    c = bwd_case(shape)
    K, D = shape[4], shape[1] // 2
    x1 = c["x"][:, D:]
    inside = (x1 >= -TB) & (x1 <= TB)
    assert torch.equal(inside, ~c["outside"])
    assert ((x1.abs() - TB).abs() >= 1e-3 * TB)[~inside].all()
    i64 = ref.bin_index(ref.knots(ref.split_params(c["h"].double(), D, K), K, TB)[0], x1.double())
    i32 = ref.bin_index(ref.knots(ref.split_params(c["h"], D, K), K, TB)[0], x1)
    assert torch.equal(i64[inside], i32[inside]) and torch.equal(i64[inside], c["k"][inside])
    assert 0.0 < c["floor"]["gx"] < 1e-2 and 0.0 < c["floor"]["gh"] < 1e-2


# ------------------------------------------------------------------------------------------ kernels: forward and inverse
def _views(shape, x, how):
    """x (dense, CPU) as a device tensor: dense, or the channel / batch slice of a larger one, or 4 bytes off 16-byte alignment."""
    B, C, H, W, _ = shape
    if how == "dense":
        return x.to(DEV)
    if how == "channel":
        big = torch.full((B, C + 8, H, W), float("nan"), device=DEV)
        big[:, 4:4 + C] = x.to(DEV)
        return big[:, 4:4 + C]
    if how == "batch":
        big = torch.full((2 * B, C, H, W), float("nan"), device=DEV)
        big[::2] = x.to(DEV)
        return big[::2]
    flat = torch.full((x.numel() + 1,), float("nan"), device=DEV)
    flat[1:] = x.to(DEV).reshape(-1)
    return flat[1:].view(B, C, H, W)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_kernel_forward_and_inverse_against_fp64(L, shape):
    """z, ldj of the forward and x, ldj of the inverse against the fp64 restatement, no element left out (the map and its
    log-derivative are C1); inverse(forward(x)) against x; the inverse's ldj against the forward's at the recovered input; two
    launches bitwise equal.  Measured figures: profiles/spline_coupling.md."""
    c = fwd_case(shape)
    K, fl = shape[4], c["floor"]
    hows = ("channel", "batch") if shape == SLICE_SHAPE else ("dense",)
    for how in hows:
        x, zi, h = _views(shape, c["x"], how), _views(shape, c["zi"], how), c["h"].to(DEV)
        z, ldj = _apply(x, h, K, False)
        xi, ldji = _apply(zi, h, K, True)
        errs = dict(z=_rel(z, c["z64"]), ldj=_rel(ldj, c["ldj64"]), xi=_rel(xi, c["xi64"]), ldji=_rel(ldji, c["ldji64"]))
        xrt, ldj_rt = _apply(z, h, K, True)
        errs["xrt"] = _rel(xrt, c["x"])
        gap = ldji - _apply(xi, h, K, False)[1]
        errs["ldjgap"] = gap.abs().max().item() / max(1.0, c["ldj64"].abs().max().item())
        for k, e in errs.items():
            print("SPLINE_FWD %s %s %s: error %.3e, fp32 floor %.3e, bar %.3e" % ("-".join(map(str, shape)), how, k, e, fl[k], _bar(fl[k])))
        for k, e in errs.items():
            assert e <= _bar(fl[k]), "%s: error %.3e (fp32 floor %.3e, bar %.3e)" % (k, e, fl[k], _bar(fl[k]))
        assert torch.equal(z[:, : shape[1] // 2], x[:, : shape[1] // 2]) and z.is_contiguous()
        z2, ldj2 = _apply(x, h, K, False)
        xi2, ldji2 = _apply(zi, h, K, True)
        assert torch.equal(z, z2) and torch.equal(ldj, ldj2) and torch.equal(xi, xi2) and torch.equal(ldji, ldji2)
        assert _apply(zi, h, K, True, ldj=False)[1] is None and torch.equal(_apply(zi, h, K, True, ldj=False)[0], xi)


@pytest.mark.gpu
def test_vector_and_scalar_forms_agree_bitwise(L):
    """The dwordx4 form (aligned, H W % 4 == 0) and the dword form (the same data 4 bytes off alignment) give the same bits,
    forward, inverse and backward."""
    shape = SLICE_SHAPE
    c, cb = fwd_case(shape), bwd_case(shape)
    K = shape[4]
    h = c["h"].to(DEV)
    for inverse in (False, True):
        a = _apply(_views(shape, c["zi" if inverse else "x"], "dense"), h, K, inverse)
        b = _apply(_views(shape, c["zi" if inverse else "x"], "offset"), h, K, inverse)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ga = _bwd(shape, cb, "dense")
    gb = _bwd(shape, cb, "offset")
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])


@pytest.mark.gpu
def test_empty_batch_and_unsupported_bins(L):
    from contextflow_amd.layers import _hip
    lib, null = _hip.lib(), _hip.p(None)
    assert lib.cf_spline_coupling(null, null, null, null, 0, 4, 4, 5, TB, 16, 0, _hip.stream()) == 0      # B = 0: pointers untouched
    assert lib.cf_spline_coupling_bwd(null, null, null, null, null, null, 0, 4, 4, 5, TB, 16, 16, _hip.stream()) == 0
    x = torch.zeros(1, 4, 2, 2, device=DEV)
    for K in (1, 17):
        h = torch.zeros(1, 2 * (3 * K - 1), 2, 2, device=DEV)
        z, ldj = torch.empty_like(x), torch.empty(1, device=DEV)
        rc = lib.cf_spline_coupling(_hip.p(x), _hip.p(h), _hip.p(z), _hip.p(ldj), 1, 4, 4, K, TB, 16, 0, _hip.stream())
        assert rc == -2                                                                                   # CF_ERR_UNSUPPORTED
        rc = lib.cf_spline_coupling_bwd(_hip.p(x), _hip.p(h), _hip.p(x), _hip.p(ldj), _hip.p(z), _hip.p(torch.empty_like(h)),
                                        1, 4, 4, K, TB, 16, 16, _hip.stream())
        assert rc == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ kernel: backward
def _bwd(shape, c, how):
    from contextflow_amd.layers import _hip
    B, C, H, W, K = shape
    x, xbs = _hip.bview(_views(shape, c["x"], how))
    gz, gzbs = _hip.bview(_views(shape, c["gz"], how))
    h, gld = c["h"].to(DEV), c["gld"].to(DEV)
    gx = torch.full((B, C, H, W), float("nan"), device=DEV)
    gh = torch.full_like(h, float("nan"))
    _hip.call("cf_spline_coupling_bwd", _hip.p(x), _hip.p(h), _hip.p(gz), _hip.p(gld), _hip.p(gx), _hip.p(gh), B, C, H * W, K, TB,
              xbs, gzbs, _hip.stream())
    return gx, gh


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_kernel_backward_against_fp64_autograd(L, shape):
    """gx = [gz0 | gz1 dz1/dx1 + gld d lad/dx1] and gh against fp64 autograd through the restatement on inputs away from every
    discontinuity of the parameter gradient (test_fp32_restatement_picks_the_fp64_bin); no element excluded.  Outside the
    tails gx1 = gz1 and gh = 0 exactly.  Measured figures: profiles/spline_coupling.md."""
    c = bwd_case(shape)
    D, fl = shape[1] // 2, c["floor"]
    hows = ("channel", "batch") if shape == SLICE_SHAPE else ("dense",)
    for how in hows:
        gx, gh = _bwd(shape, c, how)
        assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gh).all())
        for name, got in (("gx", gx), ("gh", gh)):
            want = c[name + "64"]
            e = (got.double().cpu() - want).abs().max().item() / want.abs().max().item()
            bar = min(1e-4, _bar(fl[name]))
            print("SPLINE_BWD %s %s %s: error %.3e, fp32 floor %.3e, bar %.3e" % ("-".join(map(str, shape)), how, name, e, fl[name], bar))
            assert e <= bar, "%s: error %.3e (fp32 autograd floor %.3e, bar %.3e)" % (name, e, fl[name], bar)
        out = c["outside"]
        assert torch.equal(gx[:, :D].cpu(), c["gz"][:, :D])
        assert torch.equal(gx[:, D:].cpu()[out], c["gz"][:, D:][out])
        ghe = ref.split_params(gh.cpu(), D, shape[4])
        assert not ghe[out].any()
        g2 = _bwd(shape, c, how)
        assert torch.equal(gx, g2[0]) and torch.equal(gh, g2[1])


# ------------------------------------------------------------------------------------------ layer
def _layer(L, C, krn, pad, K, seed):
    torch.manual_seed(seed)
    m = L.SplineCoupling(C, kernel_size=krn, padding=pad, bins=K, tail_bound=TB)
    with torch.no_grad():
        m.NN[4].weight.normal_(0.0, 0.4)
        m.NN[4].bias.normal_(0.0, 0.5)
    return m


def _weights(m, dt):
    return tuple(t.detach().cpu().to(dt) for t in (m.NN[0].weight, m.NN[0].bias, m.NN[2].weight, m.NN[2].bias, m.NN[4].weight, m.NN[4].bias))


@pytest.mark.gpu
def test_fresh_layer_is_the_identity(L):
    m = L.SplineCoupling(8, kernel_size=(3, 3), padding=(1, 1)).to(DEV)
    x = 1.5 * torch.randn(5, 8, 6, 6, generator=torch.Generator().manual_seed(1)).to(DEV)
    assert (x.abs() > TB).any()
    z, ldj = m(x)
    N = 4 * 36
    assert (z - x).abs().max().item() <= 1e-5 and ldj.abs().max().item() <= 1e-5 * N
    assert (m.reverse(z) - x).abs().max().item() <= 1e-5
    assert torch.equal(m.logdet(x), ldj)


@pytest.mark.gpu
@pytest.mark.parametrize("C,H,W,krn,pad,K", [(8, 6, 5, (3, 3), (1, 1), 8), (26, 8, 1, (3, 1), (1, 0), 5), (4, 4, 4, (1, 1), (0, 0), 16)])
def test_layer_against_the_restatement(L, C, H, W, krn, pad, K):
    """forward / reverse / reverse_ldj of a layer with random conditioner weights against the fp64 restatement composed with the
    oracle's conditioner (oracle.flow_oracle.coupling_net, the last convolution D (3K-1) wide)."""
    m = _layer(L, C, krn, pad, K, 3)
    B, D = 4, C // 2
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, C, H, W, generator=g)
    x[:, D:] *= 2.0
    res = {}
    for dt in (torch.float64, torch.float32):
        p = {"NN.%d.%s" % (i, n): getattr(m.NN[i], n).detach().to(dt) for i in (0, 2, 4) for n in ("weight", "bias")}
        hd = fo.coupling_net(x.to(dt)[:, :D], p, "", pad)
        z, ldj = ref.coupling_map(x.to(dt), hd, K, TB)
        xr = ref.coupling_map(z, fo.coupling_net(z[:, :D], p, "", pad), K, TB, inverse=True)[0]
        res[dt] = (z, ldj, xr)
    fz, fl, fr = (_rel(a, b) for a, b in zip(res[torch.float32], res[torch.float64][:2] + (x,)))
    m = m.to(DEV)
    z, ldj = m(x.to(DEV))
    xr, ldj_r = m.reverse_ldj(z)
    ez, el, er = _rel(z, res[torch.float64][0]), _rel(ldj, res[torch.float64][1]), _rel(xr, x)
    print("SPLINE_LAYER C=%d K=%d: z %.3e (floor %.3e)  ldj %.3e (floor %.3e)  round trip %.3e (floor %.3e)" % (C, K, ez, fz, el, fl, er, fr))
    assert ez <= _bar(fz) and el <= _bar(fl) and er <= _bar(fr)
    assert torch.equal(m.reverse(z), xr)
    # reverse_ldj: the forward log-det at the recovered input (the conditioner sees the same x0 bits in both calls)
    ldj_f = m(xr)[1]
    gap = (ldj_r - ldj_f).abs().max().item() / max(1.0, ldj_f.abs().max().item())
    assert gap <= _bar(fl), (gap, fl)


# ------------------------------------------------------------------------------------------ flows
def _data(name, B, seed):
    C, H, W = fo.CONFIGS[name][0]
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, H, W, generator=g) if name == "smap" else torch.randint(0, 256, (B, C, H, W), generator=g).float()
    u = torch.full((B, C, H, W), 0.5)
    eps = [torch.randn(B, 1, H, W, generator=g)]
    return x, u, eps


def _spline_flow(name, B=6):
    """A spline flow of the preset with initialised ActNorms (one first call on the data) and perturbed last convolutions; returns
    (model on the device, its parameters on the CPU, data, noise).
    Size of the perturbation (weights 0.1 randn, biases 0.2 randn): the raw knot parameters come out with a standard deviation
    of 0.3 and the log-derivative of an element within about [-2.2, 1.4] (the fp64 restatement on cifar10).  The round trip needs
    that: an inverse amplifies a rounding by 1 / derivative, twelve couplings in a row - at 0.3 / 0.5 the log-derivatives reach -8
    and the fp32 restatement on the CPU itself returns 2 % of the cifar10 pixels."""
    import contextflow_amd as cfa
    from tests.gpu_util import set_noise
    torch.manual_seed(11)
    cfg, data_size, M = cfa.preset_config(name, coupling="spline")
    model = cfa.create_model(cfg, data_size, M)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for m in model.sequence_modules:
            if isinstance(m, cfa.layers.SplineCoupling):
                m.NN[4].weight.copy_(0.1 * torch.randn(m.NN[4].weight.shape, generator=g))
                m.NN[4].bias.copy_(0.2 * torch.randn(m.NN[4].bias.shape, generator=g))
    model = model.to(DEV)
    x, u, eps = _data(name, B, 17)
    set_noise(model, u, eps)
    with torch.no_grad():
        model(x.to(DEV))                                     # ActNorm's data-dependent initialisation
    model.eval()
    assert all(m.is_initialized() for m in model.sequence_modules if isinstance(m, cfa.layers.ActNorm))
    params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return model, params, x, u, eps


def _restated_flow(name, params, x, u, eps, dt):
    """log p(x) (B, M) of the spline flow: oracle.flow_oracle's ops with the spline restatement in the place of the coupling."""
    ops, _, _ = fo.program(name, coupling="conv")
    p = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in params.items()}
    x, eps = x.to(dt), [e.to(dt) for e in eps]
    B, M = x.shape[0], p["dist.wG"].shape[0]
    logdet = torch.zeros(B, M, dtype=dt)
    for op in ops:
        kind, pre = op[0], "%d." % op[1]
        if kind == "dequant":
            x, ldj = x + u.to(dt), torch.zeros(B, dtype=dt)
        elif kind == "affine":
            x, ldj = fo.affine_fwd(x, op[2], op[3])
        elif kind == "logit":
            x, ldj = fo.logit_fwd(x)
        elif kind == "augment":
            e = eps.pop(0)
            x, ldj = torch.cat([x, e], 1), fo.std_normal_neg_logq(e)
        elif kind == "squeeze":
            x, ldj = fo.squeeze_fwd(x, op[2]), torch.zeros(B, dtype=dt)
        elif kind == "conv1x1":
            x, ldj = fo.conv1x1_fwd(x, p[pre + "NN"])
        elif kind == "actnorm":
            x, ldj = fo.actnorm_fwd(x, p[pre + "NN_t"], p[pre + "NN_logs"])
        elif kind == "coupling":
            K = p[pre + "NN.4.bias"].numel() // (x.shape[1] // 2)
            K = (K + 1) // 3
            x, ldj = ref.coupling_map(x, fo.coupling_net(x[:, : x.shape[1] // 2], p, pre, op[4]), K, TB)
        elif kind == "split":
            c = x.shape[1] // 2
            ldj = fo.gmm_logprob(x[:, c:], p[pre + "dist.mG"], p[pre + "dist.sG"], p[pre + "dist.wG"])
            x = x[:, :c]
        else:
            raise ValueError(kind)
        logdet = logdet + (ldj if ldj.dim() == 2 else ldj.unsqueeze(-1))
    return fo.gmm_logprob(x, p["dist.mG"], p["dist.sG"], p["dist.wG"]) + logdet


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mnist", "cifar10", "smap"])
def test_spline_flow_plan_round_trip_and_sampling(L, name):
    """The fused plan (Conv1x1, ActNorm and SplineCoupling as layer records between the fused pre-processing and mixture
    kernels) against the layer-by-layer walk, at the bar tests/test_gpu_parity.py holds those two paths to; both against the fp64
    restatement of the flow; decode(encode(x)) returns the pixels; decode's logp against encode's; sample returns (n, M)."""
    model, params, x, u, eps = _spline_flow(name)
    D = x[0].numel()
    xd = x.to(DEV)
    with torch.no_grad():
        assert model._fusable()
        _, lp = model(xd)
        _, lp_layers = model._forward_layers(xd, None)
    assert (lp - lp_layers).abs().max().item() / D < 2 * BPD_TOL
    lp64 = _restated_flow(name, params, x, u, eps, torch.float64)
    lp32 = _restated_flow(name, params, x, u, eps, torch.float32)
    entries = lambda t: -t.double() / (D * math.log(2.0))
    floor = (entries(lp32) - entries(lp64)).abs().max().item()
    e = (entries(lp.cpu()) - entries(lp64)).abs().max().item()
    bar = max(BPD_TOL, 3.0 * floor)
    print("SPLINE_FLOW %s log_prob vs fp64: %.3e bits/dim per entry (fp32 floor %.3e, bar %.3e)" % (name, e, floor, bar))
    assert e <= bar
    assert (bpd(lp.cpu(), name) - bpd(lp64, name)).abs().max().item() <= bar
    latents, lp_enc = model.encode(xd)
    assert torch.equal(lp_enc, lp)
    xr, lp_dec = model.decode(latents, return_logp=True)
    if name != "smap":
        assert torch.equal(xr.cpu(), x)                      # every pixel (dequantisation noise 0.5)
        assert torch.equal(model.decode(latents), xr)
    ed = (entries(lp_dec.cpu()) - entries(lp_enc.cpu())).abs().max().item()
    print("SPLINE_FLOW %s decode(return_logp) vs encode: %.3e bits/dim per entry (bar %.3e)" % (name, ed, bar))
    assert tuple(lp_dec.shape) == tuple(lp_enc.shape) and ed <= bar
    torch.manual_seed(3)
    xs, lps = model.sample(9, return_logp=True)
    assert tuple(xs.shape) == (9,) + tuple(x.shape[1:]) and tuple(lps.shape) == (9, lp.shape[1])
    assert bool(torch.isfinite(xs).all()) and bool(torch.isfinite(lps).all())


@pytest.mark.gpu
def test_small_flow_score_and_parameter_gradients_against_fp64_autograd(L):
    """FlowSequential(GaussianMixtureDistribution((4, 4, 4), 2, 8), Conv1x1, ActNorm, SplineCoupling(4, (3, 3), (1, 1), bins=5)), B = 3:
    score(x) and every parameter gradient of log_prob(x).sum() against fp64 autograd through the oracle's pieces and the spline
    restatement; error = max|got - ref| / max|ref| per tensor, bar max(1e-4, 3 x the error of fp32 autograd): tests/test_score.py."""
    torch.manual_seed(2)
    model = L.FlowSequential(L.GaussianMixtureDistribution((4, 4, 4), 2, 8), L.Conv1x1((4, 4, 4)), L.ActNorm((4, 4, 4)),
                             L.SplineCoupling(4, (3, 3), (1, 1), bins=5))
    with torch.no_grad():
        model.sequence_modules[2].NN[4].weight.normal_(0.0, 0.4)
        model.sequence_modules[2].NN[4].bias.normal_(0.0, 0.5)
    model = model.to(DEV)
    x = 1.5 * torch.randn(3, 4, 4, 4, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        model(x.to(DEV))                                     # ActNorm init
    params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    names = [k for k, _ in model.named_parameters()]

    def restated(dt):
        p = {k: v.to(dt).clone().requires_grad_(True) for k, v in params.items() if v.is_floating_point()}
        xx = x.to(dt).clone().requires_grad_(True)
        y, l0 = fo.conv1x1_fwd(xx, p["0.NN"])
        y, l1 = fo.actnorm_fwd(y, p["1.NN_t"], p["1.NN_logs"])
        y, l2 = ref.coupling_map(y, fo.coupling_net(y[:, :2], p, "2.", (1, 1)), 5, TB)
        lp = fo.gmm_logprob(y, p["dist.mG"], p["dist.sG"], p["dist.wG"]) + (l0 + l1 + l2).unsqueeze(-1)
        sc = torch.autograd.grad(torch.logsumexp(lp, dim=1).sum(), xx, retain_graph=True)[0]      # score(x): of the marginal
        lp.sum().backward()
        return lp.detach(), sc, {k: p[k].grad for k in names}
    lp64, gx64, gp64 = restated(torch.float64)
    _, gx32, gp32 = restated(torch.float32)
    model.train()
    for prm in model.parameters():
        prm.grad = None
    _, lp = model(x.to(DEV))
    assert (lp.detach().cpu().double() - lp64).abs().max().item() <= 2e-5 * max(1.0, lp64.abs().max().item())
    lp.sum().backward()
    got = {k: prm.grad for k, prm in model.named_parameters()}
    model.eval()
    score, _ = model.score(x.to(DEV))
    checks = [("score", score, gx64, gx32)] + [(k, got[k], gp64[k], gp32[k]) for k in names]
    worst = []
    for k, g_, r64, r32 in checks:
        assert g_ is not None and r64 is not None, k
        scale = r64.abs().max().item()
        floor = (r32.double() - r64).abs().max().item() / scale
        e = (g_.double().cpu().reshape(r64.shape) - r64).abs().max().item() / scale
        bar = max(1e-4, 3.0 * floor)
        print("SPLINE_SMALL %s: relative error %.3e, fp32 floor %.3e, bar %.3e" % (k, e, floor, bar))
        if e > bar:
            worst.append((k, e, floor, bar))
    assert not worst, worst


@pytest.mark.gpu
def test_training_lowers_the_loss(L):
    """Twenty AdamW steps on the mnist spline flow at B = 32."""
    import contextflow_amd as cfa
    from tests.gpu_util import set_noise
    torch.manual_seed(4)
    cfg, data_size, M = cfa.preset_config("mnist", coupling="spline")
    model = cfa.create_model(cfg, data_size, M).to(DEV)
    g = torch.Generator().manual_seed(9)
    base = torch.randint(0, 256, (1, 1, 32, 32), generator=g).float()
    x = (base + torch.randint(-20, 21, (32, 1, 32, 32), generator=g)).clamp(0, 255).to(DEV)
    set_noise(model, torch.rand(32, 1, 32, 32, generator=g), [torch.randn(32, 1, 32, 32, generator=g)])
    with torch.no_grad():
        model(x)
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        _, lp = model(x)
        loss = -torch.logsumexp(lp, dim=-1).mean() / (32 * 32 * math.log(2.0))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("SPLINE_TRAIN mnist B=32: bits/dim %.4f -> %.4f" % (losses[0], losses[-1]))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    assert any(p.grad is not None and bool(p.grad.abs().sum() > 0) for m in model.sequence_modules
               if isinstance(m, cfa.layers.SplineCoupling) for p in m.NN[4].parameters())
