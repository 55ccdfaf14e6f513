"""The backward of the fused conv flow step ([Squeeze ->] Conv1x1 -> ActNorm -> Coupling) against fp64 torch.autograd on EVERY
branch of the dispatch: which kernels tape the forward (select(Pass::Taped, ...)) and run the backward (cf_flow_step_bwd_taped)
depends on the batch size, and only the smallest-batch branch of each level is reached by whole-model comparisons.  The
reference (tests/step_fp64_ref.py) is one step over oracle/flow_oracle.py with the ReLU masks as arguments: the planes and
outputs are held against the true-ReLU fp64 run, the masks may differ from its masks only within rounding of zero, and the
gradients are compared under the KERNEL's masks (read from the tape's h1 / h2 planes - the kernel itself reads the aux words,
so a disagreement between the two shows here).  Bar per tensor: min(1e-4, max(2e-6, 4 x the error of fp32 torch.autograd on
the CPU under the same masks)).  Measured errors: profiles/step_backward_fp64.md.

The tests without the `gpu` mark run the reference, the floors and the preconditions on the inputs of every case on the CPU,
and show that restated defects (a sample dropped from a weight gradient, a mask plane of the other layer, gld ignored) break
the bars.  The file passes with the default dispatch and with CONTEXTFLOW_DIRECT_CONV=1."""
import functools
import os

import pytest
import torch

from oracle import flow_oracle as fo
from tests import step_fp64_ref as R

DEV = "cuda:0"
DIRECT = os.environ.get("CONTEXTFLOW_DIRECT_CONV", "")[:1] == "1"
ids = lambda cases: [c.id for c in cases]


def close(a, b, tol=1e-5):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item()
    assert err <= tol * scale, "max err %.3e (scale %.3e)" % (err, scale)


@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


@functools.lru_cache(maxsize=2)
def _drawn(case):
    """(inputs, true-ReLU fp64 run with its gradients) of a case: computed once, read-only."""
    d = R.draw(case)
    return d, R.step_ref(d, case.squeeze, case.mode)


def _report(case, what, **kv):
    print("REPORT|%s|%s|%s" % (case.id, what, "|".join("%s=%s" % (k, ("%.3e" % v) if isinstance(v, float) else v) for k, v in kv.items())))


def _check_band(case, ref):
    s1, s2, share, n = R.band_share(ref)
    if case.mode == 1:
        assert n == 0, "%s: %d units inside the band - pick another seed" % (case.id, n)
    assert share <= R.BAND_MAX, "%s: %.2e of the ReLU units inside the band" % (case.id, share)
    return share, n


def _compare(case, got, refm, floor):
    """got / refm: {name: tensor}; every tensor of R.grad_names(case.mode) finite and within its bar."""
    failed = []
    for k in R.grad_names(case.mode):
        assert torch.isfinite(got[k]).all(), (case.id, k)
        err, b = R.rel_err(got[k], refm[k]), R.bar(floor[k])
        _report(case, k, err=err, floor=floor[k], bar=b)
        if not err <= b:
            failed.append("%s: err %.3e > bar %.3e (floor %.3e)" % (k, err, b, floor[k]))
    assert not failed, (case.id, failed)


# ================================================================================================ CPU: reference, floors, inputs
@pytest.mark.parametrize("case", [R.Case(8, 16, 2), R.Case(16, 16, 2, squeeze=1), R.Case(32, 8, 3, sliced=1), R.Case(64, 4, 5, squeeze=1, sliced=1),
                                  R.Case(16, 16, 2, mode=1), R.Case(32, 8, 3, mode=2)], ids=lambda c: c.id)
def test_reference_equals_autograd_through_the_oracle(case):
    """step_ref with the true ReLU = torch.autograd through fo.coupling_fwd o fo.actnorm_fwd o fo.conv1x1_fwd [o fo.squeeze_fwd]
    (specialist modes: fo.coupling_net with CN(c) placed as fo.coupling_ctx_fwd places it) in fp64, to 1e-12: outputs, the tape
    planes' sources, dL/dx and every parameter gradient."""
    d = R.draw(case)
    ref = R.step_ref(d, case.squeeze, case.mode)
    C, B, H = case.C, case.B, case.H
    lv = lambda t: t.detach().double().clone().requires_grad_()
    p = {k: lv(v) for k, v in d["p"].items()}
    x, gz, gld = lv(d["x"]), d["gz"].double(), d["gld"].double()
    y = fo.squeeze_fwd(x, (2, 2)) if case.squeeze else x
    if case.mode == 0:
        y, l0 = fo.conv1x1_fwd(y, p["Conv1x1.NN"])
        y, l1 = fo.actnorm_fwd(y, p["ActNorm.NN_t"], p["ActNorm.NN_logs"])
        z, l2 = fo.coupling_fwd(y, {"0." + k: v for k, v in p.items()}, "0.", (1, 1))
        ld = l0 + l1 + l2
    elif case.mode == 1:                 # contextflow: h = NN(x0) + CN(c)
        sb = lv(d["sbias"])
        h = fo.coupling_net(y[:, : C // 2], {"0." + k: v for k, v in p.items()}, "0.", (1, 1)) + sb.view(B, -1, 1, 1)
        z, ld = fo.coupling_apply_fwd(y, h)
    else:                                # CN(c) broadcast and concatenated to the conditioner input: sbias = W[:, D:] CN(c)
        g = torch.Generator().manual_seed(5)
        wc, cn = torch.randn(2 * C, C, generator=g).double(), torch.randn(B, C, generator=g).double()
        d = dict(d, sbias=cn @ wc.t())
        ref = R.step_ref(d, case.squeeze, case.mode)
        q = {"0." + k: v for k, v in p.items()}
        q["0.NN.0.weight"] = torch.cat([p["NN.0.weight"], wc.view(2 * C, C, 1, 1)], 1)
        sb = lv(cn)
        xin = torch.cat([y[:, : C // 2], sb.view(B, -1, 1, 1).expand(B, C, H, H)], 1)
        z, ld = fo.coupling_apply_fwd(y, fo.coupling_net(xin, q, "0.", (1, 1)))
    ((z * gz).sum() + (ld * gld).sum()).backward()
    want = dict(z=z.detach(), ld=ld.detach(), gx=x.grad, **{k: v.grad for k, v in p.items()})
    if case.mode == 1:
        want["gsbias"] = sb.grad
    if case.mode == 2:                   # d/d CN(c) = (d/d sbias) W[:, D:]
        assert R.rel_err(ref["gsbias"] @ wc, sb.grad) <= 1e-12
    for k, w in want.items():
        assert R.rel_err(ref[k], w) <= 1e-12, (k, R.rel_err(ref[k], w))


@pytest.mark.parametrize("case", R.CASES, ids=ids(R.CASES))
def test_reference_preconditions_and_floor(case):
    """Per case, without a GPU: the share of ReLU units of the fp64 run inside the band is <= 1e-4 (mode 1: none at all); with the
    masks of fp32 torch.autograd on the CPU in the kernel's place every mask that differs lies inside the band; the floor (fp32
    against fp64 under those masks) leaves the bar below the 1e-4 cap for every tensor."""
    d, ref = _drawn(case)
    share, n = _check_band(case, ref)
    r32 = R.step_ref(d, case.squeeze, case.mode, dtype=torch.float32, grads=False)
    m1, m2 = (r32["h1"] > 0, r32["h2"] > 0) if case.mode != 1 else (ref["a1"] > 0, ref["a2"] > 0)
    ndiff, bad = R.mask_disagreements(ref, m1, m2)
    assert bad == 0, (case.id, ndiff, bad)
    refm, floor = R.floors(d, case, m1, m2)
    _report(case, "cpu", share=share, in_band=n, masks_differ=ndiff, **{k: float(v) for k, v in floor.items()})
    for k, v in floor.items():
        assert v <= R.GRAD_CAP / R.FLOOR_FACTOR, (case.id, k, v)


DEFECT_CASES = [c for c in R.GENERALIST if (c.C, c.B) in ((8, 67), (16, 67), (32, 513), (32, 1027), (64, 7), (64, 1537), (64, 2051))
                and not c.squeeze] + [R.MODE2[-1]]


@pytest.mark.parametrize("case", DEFECT_CASES, ids=ids(DEFECT_CASES))
def test_restated_defects_break_the_bar(case):
    """The comparison can fail: three defects restated on the CPU (in fp64, so nothing but the defect differs) against the bars
    the GPU test uses for the case.  (a) the last sample - the ragged last workgroup's - missing from the three conv weight
    gradients; (b) the backward reads the mask plane of the OTHER layer; (c) gld ignored.  Each must exceed the bar of the tensors
    it touches; the factors go to profiles/step_backward_fp64.md."""
    d, ref = _drawn(case)
    m1, m2 = ref["a1"] > 0, ref["a2"] > 0
    refm, floor = R.floors(d, case, m1, m2, ref=ref)
    names = R.grad_names(case.mode)
    factor = lambda got, k: R.rel_err(got, refm[k]) / R.bar(floor[k])
    # (a) one sample dropped: the weight gradients are sums over samples, so the defect is the last sample's own term
    last = dict(d, x=d["x"][-1:], gz=d["gz"][-1:], gld=d["gld"][-1:], sbias=None if d["sbias"] is None else d["sbias"][-1:])
    own = R.step_ref(last, case.squeeze, case.mode, m1[-1:], m2[-1:])
    fa = {k: factor(refm[k] - own[k], k) for k in ("NN.0.weight", "NN.2.weight", "NN.4.weight")}
    # (b) masks swapped in the backward only (same shape (B, 2C, H, W) for both layers)
    sw = R.step_ref(d, case.squeeze, case.mode, m1, m2, bwd_masks=(m2, m1))
    fb = {k: factor(sw[k], k) for k in names}
    # (c) gld ignored
    ng = R.step_ref(dict(d, gld=torch.zeros_like(d["gld"])), case.squeeze, case.mode, m1, m2)
    fc = {k: factor(ng[k], k) for k in names}
    for tag, f in (("drop_last_sample", fa), ("mask_of_other_layer", fb), ("gld_ignored", fc)):
        _report(case, "defect:" + tag, **{k: float(v) for k, v in f.items()})
    assert min(fa.values()) > 1, fa
    # the swapped mask reaches everything behind the second ReLU's adjoint; NN.4 and the last bias lie in front of it
    assert all(fb[k] > 1 for k in names if k not in ("NN.4.weight", "NN.4.bias")), fb
    # gld enters through d ld / d log_s (every conditioner tensor and dL/dx) and through the Conv1x1 / ActNorm log-dets; the
    # ActNorm shift sees it only through the conditioner as well
    assert all(fc[k] > 1 for k in names), fc


# ================================================================================================ GPU
def _modules(L, case, p):
    C, H = case.C, case.H
    cpl = L.Coupling(C, kernel_size=(3, 3), padding=(1, 1))
    with torch.no_grad():
        for i in (0, 2, 4):
            cpl.NN[i].weight.copy_(p["NN.%d.weight" % i]); cpl.NN[i].bias.copy_(p["NN.%d.bias" % i])
    if case.mode:
        return None, None, cpl.to(DEV)
    conv, act = L.Conv1x1((C, H, H)), L.ActNorm((C, H, H))
    with torch.no_grad():
        conv.NN.copy_(p["Conv1x1.NN"]); act.NN_t.copy_(p["ActNorm.NN_t"]); act.NN_logs.copy_(p["ActNorm.NN_logs"]); act.initialized.fill_(1)
    act._init_done = True
    return conv.to(DEV), act.to(DEV), cpl.to(DEV)


def _device_x(d):
    if d["big"] is not None:             # the SplitPrior case: the first half of the channels, read in place
        return d["big"].to(DEV)[:, : d["x"].shape[1]]
    return d["x"].to(DEV)


def _planes_and_masks(case, ref, z, ld, planes):
    """Forward outputs and tape planes against the true-ReLU fp64 run (1e-5 of scale, the bars of test_fused_step_phases); the
    kernel's masks from its planes; every mask that differs from the fp64 run's inside the band."""
    B, C, H = case.B, case.C, case.H
    close(z, ref["z"]); close(ld, ref["ld"])
    for k, pl, rows in (("y0", planes[0], C // 2), ("h1", planes[1], 2 * C), ("h2", planes[2], 2 * C)):
        close(pl.view(B, rows, H, H), ref[k])
    m1, m2 = (planes[1] > 0).view(B, 2 * C, H, H).cpu(), (planes[2] > 0).view(B, 2 * C, H, H).cpu()
    ndiff, bad = R.mask_disagreements(ref, m1, m2)
    share, n = _check_band(case, ref)
    _report(case, "masks", differ=ndiff, outside_band=bad, in_band=n, share=share)
    assert bad == 0, "%s: %d of %d differing mask bits lie outside the band" % (case.id, bad, ndiff)
    return m1, m2


def _winograd_taped(case):
    """Does the taping forward of this generalist case run a Winograd form of the 3x3 (select(Pass::Taped, ...))?"""
    if DIRECT:
        return False
    return {8: False,                                    # Small_G8s: direct at every batch
            16: True,                                    # Small_G16w at every batch
            32: case.B >= 1024,                          # kFullMinB8x8
            64: case.B >= 2048}[case.C]                  # kWinoMinB4x4


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.GENERALIST, ids=ids(R.GENERALIST))
def test_step_backward_against_fp64(L, case):
    """cf_flow_step_fwd_taped -> autograd.step_backward (cf_flow_step_bwd_taped, cf_step_wgrads_batch, cf_step_param_grads_batch):
    z, ld, y0, h1, h2 against the true-ReLU fp64 run; the masks; dL/dx and the nine parameter gradients against the fp64 run under
    the kernel's masks; cf_flow_step_bwd_data bitwise equal in dL/dx."""
    from contextflow_amd.layers import _hip, _tape, autograd
    lib, P, st = _hip.lib(), _hip.p, _hip.stream()
    d, ref = _drawn(case)
    B, C, H, sq = case.B, case.C, case.H, case.squeeze
    HW = H * H
    assert lib.cf_flow_step_macs(B, C, H, H, 1) == (20 if _winograd_taped(case) else 40) * C * C * HW
    conv, act, cpl = _modules(L, case, d["p"])
    f = lambda t: _hip.f32(t.detach())
    c1, c2, c3 = cpl.NN[0], cpl.NN[2], cpl.NN[4]
    ws = torch.empty(lib.cf_flow_step_ws_bytes(C, H, H), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_prepare", P(f(conv.NN)), P(f(act.NN_t)), P(f(act.NN_logs)), P(f(c1.weight)), P(f(c1.bias)), P(f(c2.weight)),
              P(f(c2.bias)), P(f(c3.weight)), P(f(c3.bias)), P(ws), C, H, H, st)
    x = _device_x(d)
    xv, xbs = _hip.bview(x)
    assert xv.data_ptr() == x.data_ptr() and xbs == (2 if case.sliced else 1) * C * HW
    z, ld = torch.full((B, C, H, H), float("nan"), device=DEV), torch.zeros(B, device=DEV)
    planes = _tape.step_tape(B, C, H, H, DEV)
    _hip.call("cf_flow_step_fwd_taped", P(xv), P(z), P(ld), P(ws), P(planes[0]), P(planes[1]), P(planes[2]), P(planes[3]), B, C, H, H,
              xbs, sq, st)
    m1, m2 = _planes_and_masks(case, ref, z, ld, planes)
    refm, floor = R.floors(d, case, m1, m2)
    gz, gld = d["gz"].to(DEV), d["gld"].to(DEV)
    rec = _tape.Step(conv, act, cpl, (C, H, H), sq, x=x, ws=ws, planes=planes)
    gx, grads = autograd.step_backward(rec, gz, gld)
    assert gx.shape == d["x"].shape
    got = {"gx": gx, "Conv1x1.NN": grads[conv.NN], "ActNorm.NN_t": grads[act.NN_t], "ActNorm.NN_logs": grads[act.NN_logs]}
    for i, c in ((0, c1), (2, c2), (4, c3)):
        got["NN.%d.weight" % i], got["NN.%d.bias" % i] = grads[c.weight], grads[c.bias]
    _compare(case, got, refm, floor)
    # the frozen-weights path on the same aux buffer
    wsb = torch.empty(lib.cf_flow_step_bwd_ws_bytes(C, H, H), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_bwd_prepare", P(f(conv.NN)), P(f(act.NN_logs)), P(f(c1.weight)), P(f(c2.weight)), P(f(c3.weight)), P(wsb), C, H, H, st)
    gxd = torch.full_like(gx, float("nan"))
    _hip.call("cf_flow_step_bwd_data", P(gz), P(gld), P(wsb), P(planes[3]), P(gxd), B, C, H, H, sq, st)
    assert torch.equal(gxd, gx)


def _ctx_tables(L, case, cpl):
    """Forward and backward tables of a specialist coupling: identity Conv1x1 / ActNorm in front (coupling.identity_front_step_tables,
    autograd_ctx._coupling_wsb)."""
    from contextflow_amd.layers import _hip
    from contextflow_amd.layers.coupling import identity_front_step_tables
    C, H = case.C, case.H
    f, P = (lambda t: _hip.f32(t.detach())), _hip.p
    ws = identity_front_step_tables(cpl, f(cpl.NN[0].weight), C, H, H, torch.device(DEV))
    wsb = torch.empty(_hip.lib().cf_flow_step_bwd_ws_bytes(C, H, H), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_bwd_prepare", P(torch.eye(C, device=DEV)), P(torch.zeros(C, device=DEV)), P(f(cpl.NN[0].weight)),
              P(f(cpl.NN[2].weight)), P(f(cpl.NN[4].weight)), P(wsb), C, H, H, _hip.stream())
    return ws, wsb


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.MODE2, ids=ids(R.MODE2))
def test_ctx_taped_step_backward_against_fp64(L, case):
    """Specialist coupling with CN(c) in front of the first ReLU: cf_flow_step_fwd_ctx_taped (Step_G*: 16 samples per workgroup at
    4x4) -> cf_flow_step_bwd_taped (rs16 at B = 19, the 8-sample tile form at B = 1541) -> cf_wgrad, as
    autograd_ctx.coupling_ctx_backward forms them, d/d sbias = per-sample row sums of s_gh1 included.  Method of
    test_step_backward_against_fp64."""
    from contextflow_amd.layers import _hip, _tape
    lib, P, st = _hip.lib(), _hip.p, _hip.stream()
    d, ref = _drawn(case)
    B, C, H = case.B, case.C, case.H
    HW, HID = H * H, 2 * C
    _, _, cpl = _modules(L, case, d["p"])
    ws, wsb = _ctx_tables(L, case, cpl)
    x, sb = d["x"].to(DEV), d["sbias"].to(DEV)
    z, ld = torch.full((B, C, H, H), float("nan"), device=DEV), torch.zeros(B, device=DEV)
    planes = _tape.step_tape(B, C, H, H, DEV)
    _hip.call("cf_flow_step_fwd_ctx_taped", P(x), P(z), P(ld), P(ws), P(sb), P(planes[0]), P(planes[1]), P(planes[2]), P(planes[3]),
              B, C, H, H, C * HW, st)
    m1, m2 = _planes_and_masks(case, ref, z, ld, planes)
    refm, floor = R.floors(d, case, m1, m2)
    gz, gld = d["gz"].to(DEV), d["gld"].to(DEV)
    new = lambda rows: torch.full((B, rows, HW), float("nan"), device=DEV)
    gx = torch.full((B, C, H, H), float("nan"), device=DEV)
    s_gh, s_gh2, s_gh1, s_gy = new(C), new(HID), new(HID), new(C)
    _hip.call("cf_flow_step_bwd_taped", P(gz), P(gld), P(wsb), P(planes[3]), P(gx), P(s_gh), P(s_gh2), P(s_gh1), P(s_gy), B, C, H, H, 0, st)

    def wgrad(A, Bm, taps):
        MR, NR = A.shape[1], Bm.shape[1]
        gw, gb = torch.full((taps, MR, NR), float("nan"), device=DEV), torch.full((MR,), float("nan"), device=DEV)
        wsw = torch.empty(lib.cf_wgrad_ws_bytes(B, MR, NR, H, H, taps), device=DEV, dtype=torch.uint8)
        _hip.call("cf_wgrad", P(A), P(Bm), P(gw), P(gb), P(wsw), B, MR, NR, H, H, taps, st)
        return gw, gb

    gw3, gb3 = wgrad(s_gh, planes[2], 1)
    gw2, gb2 = wgrad(s_gh2, planes[1], 9)
    gw1, gb1 = wgrad(s_gh1, planes[0], 1)
    gsb = torch.full((B, HID), float("nan"), device=DEV)
    _hip.call("cf_sample_channel_sums", P(s_gh1), P(gsb), B, HID, HW, st)
    got = {"gx": gx, "gsbias": gsb, "NN.0.weight": gw1[0], "NN.0.bias": gb1, "NN.2.weight": gw2.permute(1, 2, 0).reshape(HID, HID, 3, 3),
           "NN.2.bias": gb2, "NN.4.weight": gw3[0], "NN.4.bias": gb3}
    _compare(case, got, refm, floor)
    gxd = torch.full_like(gx, float("nan"))
    _hip.call("cf_flow_step_bwd_data", P(gz), P(gld), P(wsb), P(planes[3]), P(gxd), B, C, H, H, 0, st)
    assert torch.equal(gxd, gx)


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.MODE1, ids=ids(R.MODE1))
def test_ctx_recompute_step_backward_against_fp64(L, case):
    """Specialist coupling under contextflow (CN(c) on the conditioner output, conditioner frozen): cf_flow_step_fwd_ctx with
    mode | 4 -> cf_flow_step_bwd_ctx (k_flow_step_bwd<..., CTX>), which rebuilds the conditioner and writes only s_gh, so its masks
    cannot be read back: the inputs have NO unit inside the band (asserted), and dL/dx and d/d sbias = sum_p s_gh are compared with
    the true-ReLU fp64 run, no mask imposed.  cf_flow_step_bwd_ctx_data: dL/dx bitwise equal."""
    from contextflow_amd.layers import _hip
    P, st = _hip.p, _hip.stream()
    d, ref = _drawn(case)
    B, C, H = case.B, case.C, case.H
    HW = H * H
    share, n = _check_band(case, ref)
    _, _, cpl = _modules(L, case, d["p"])
    ws, wsb = _ctx_tables(L, case, cpl)
    x, sb = d["x"].to(DEV), d["sbias"].to(DEV)
    z, ld = torch.full((B, C, H, H), float("nan"), device=DEV), torch.zeros(B, device=DEV)
    _hip.call("cf_flow_step_fwd_ctx", P(x), P(z), P(ld), P(ws), P(sb), 1 | 4, B, C, H, H, C * HW, st)
    close(z, ref["z"]); close(ld, ref["ld"])
    _, floor = R.floors(d, case, ref["a1"] > 0, ref["a2"] > 0, ref=ref)
    gz, gld = d["gz"].to(DEV), d["gld"].to(DEV)
    gx, s_gh = torch.full((B, C, H, H), float("nan"), device=DEV), torch.full((B, C, HW), float("nan"), device=DEV)
    _hip.call("cf_flow_step_bwd_ctx", P(x), P(gz), P(gld), P(ws), P(wsb), P(sb), P(gx), None, None, None, P(s_gh), None, None, None,
              B, C, H, H, C * HW, st)
    gsb = torch.full((B, C), float("nan"), device=DEV)
    _hip.call("cf_sample_channel_sums", P(s_gh), P(gsb), B, C, HW, st)
    _report(case, "masks", in_band=n, share=share)
    _compare(case, {"gx": gx, "gsbias": gsb}, ref, floor)
    gxd = torch.full_like(gx, float("nan"))
    _hip.call("cf_flow_step_bwd_ctx_data", P(x), P(gz), P(gld), P(ws), P(wsb), P(sb), P(gxd), B, C, H, H, C * HW, st)
    assert torch.equal(gxd, gx)
