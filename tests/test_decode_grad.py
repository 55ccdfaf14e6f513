"""`inverse` / `decode` with differentiable=True: the latent gradient of the backward walk.

CPU: the reference of the inverse step's vector-Jacobian product (tests/decode_grad_util.py::step_inv_ref) against the existing
forward reference with no kernel involved (J_F^T J_F^-T = I), the ReLU band of every kernel case, the ABI.  GPU: the VJP kernel
per geometry, the tail kernel, the layer-path coupling rule, the whole chain of the mnist and cifar10 fixtures against fp64
autograd through the oracle's inverse, and the semantics of the flag."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import flow_oracle as fo
from tests import decode_grad_util as U
from tests import step_fp64_ref as R
from tests.sample_logp_util import problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NEW_SYMBOLS = ("cf_flow_step_inv_bwd_ws_bytes", "cf_flow_step_inv_bwd_prepare", "cf_flow_step_inv_bwd_data", "cf_postprocess_inv_bwd")
ALPHA32 = float(torch.tensor(fo.ALPHA, dtype=torch.float32))
S2_32 = float(torch.tensor(1 / (1 - 2 * fo.ALPHA), dtype=torch.float32))
ids = lambda cases: [c.id for c in cases]


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", U.CASES, ids=ids(U.CASES))
def test_step_inv_ref_inverts_the_forward_reference(case):
    """1. gz = VJP_inv(gx) by autograd through step_inv_ref at z = step_ref(x); then step_ref's gx under upstream gz with gld = 0
    returns the drawn gx (J_F^T J_F^-T = I): 1e-10 relative, fp64, no kernel involved.  x is recovered to 1e-12 on the way."""
    d, ref = U.drawn(case)
    inv = U.step_inv_ref(d, ref["z"], gx=d["gz"])
    assert R.rel_err(inv["x"], d["x"].double()) < 1e-12
    back = R.step_ref(dict(d, gz=inv["gz"], gld=torch.zeros_like(d["gld"])))
    err = R.rel_err(back["gx"], d["gz"].double())
    print("%s: J_F^T J_F^-T gx against gx, fp64: %.2e relative" % (case.id, err))
    assert err < 1e-10


@pytest.mark.parametrize("case", U.CASES, ids=ids(U.CASES))
def test_kernel_inputs_stay_clear_of_the_relu_band(case):
    """2. The kernel's masks cannot be read back: the fp64 run of every kernel case has NO unit inside step_fp64_ref.in_band."""
    _, ref = U.drawn(case)
    assert R.band_share(ref)[3] == 0, "%s: units inside the band - pick another seed" % case.id


def test_abi_of_the_new_entry_points():
    """3. Declared in the header, present in _hip's signature table, exported by the built library; the ABI version stays."""
    import ctypes
    import re
    from contextflow_amd import build
    from contextflow_amd.layers import _hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "contextflow_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.build())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, src), s
        assert s in _hip.SIGNATURES and hasattr(lib, s), s
    assert "#define CF_ABI_VERSION 16" in src and _hip.ABI_VERSION == 16
    for C, H in ((8, 16), (16, 16), (32, 8), (64, 4)):
        assert _hip.lib().cf_flow_step_inv_bwd_ws_bytes(C, H, H) >= 4 * C * C
    assert _hip.lib().cf_flow_step_inv_bwd_ws_bytes(26, 8, 1) == 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


def _step_modules(L, case, p):
    C, H = case.C, case.H
    conv, act, cpl = L.Conv1x1((C, H, H)), L.ActNorm((C, H, H)), L.Coupling(C, kernel_size=(3, 3), padding=(1, 1))
    with torch.no_grad():
        for i in (0, 2, 4):
            cpl.NN[i].weight.copy_(p["NN.%d.weight" % i]); cpl.NN[i].bias.copy_(p["NN.%d.bias" % i])
        conv.NN.copy_(p["Conv1x1.NN"]); act.NN_t.copy_(p["ActNorm.NN_t"]); act.NN_logs.copy_(p["ActNorm.NN_logs"]); act.initialized.fill_(1)
    act._init_done = True
    return conv.to(DEV), act.to(DEV), cpl.to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("case", U.CASES, ids=ids(U.CASES))
def test_step_inv_bwd_data_per_geometry(L, case):
    """4. cf_flow_step_inv_bwd_data at the exact step input x (dense, and a channel slice of a wider tensor) under the drawn gx,
    against fp64 autograd through step_inv_ref: bar = step_fp64_ref.bar(error of fp32 CPU autograd on the same graph); the
    sentinels framing gz intact; two launches the same bits.
    Measured on an MI355X: 1.6e-7 .. 5.0e-7 against floors of 1.7e-7 .. 9.1e-7 (profiles/decode_grad.md)."""
    from contextflow_amd.layers import _hip
    lib, P, st = _hip.lib(), _hip.p, _hip.stream()
    d, ref = U.drawn(case)
    B, C, H = case.B, case.C, case.H
    HW = H * H
    gx = d["gz"]
    want = U.step_inv_ref(d, ref["z"], gx=gx)["gz"]
    floor = U.step_inv_floor(d, ref["z"], gx, want)
    conv, act, cpl = _step_modules(L, case, d["p"])
    f = lambda t: _hip.f32(t.detach())
    c1, c2, c3 = cpl.NN[0], cpl.NN[2], cpl.NN[4]
    ws = torch.empty(lib.cf_flow_step_ws_bytes(C, H, H), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_prepare", P(f(conv.NN)), P(f(act.NN_t)), P(f(act.NN_logs)), P(f(c1.weight)), P(f(c1.bias)), P(f(c2.weight)),
              P(f(c2.bias)), P(f(c3.weight)), P(f(c3.bias)), P(ws), C, H, H, st)
    wsb = torch.empty(lib.cf_flow_step_bwd_ws_bytes(C, H, H), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_bwd_prepare", P(f(conv.NN)), P(f(act.NN_logs)), P(f(c1.weight)), P(f(c2.weight)), P(f(c3.weight)), P(wsb), C, H, H, st)
    wsi = torch.empty(lib.cf_flow_step_inv_ws_bytes(C, H, H), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_inv_prepare", P(f(conv.NN)), P(f(act.NN_t)), P(f(act.NN_logs)), P(wsi), C, H, H, st)
    wsv = torch.empty(lib.cf_flow_step_inv_bwd_ws_bytes(C, H, H), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_inv_bwd_prepare", P(wsi), P(f(act.NN_logs)), P(wsv), C, H, H, st)
    x = d["big"].to(DEV)[:, :C] if d["big"] is not None else d["x"].to(DEV)
    xv, xbs = _hip.bview(x)
    assert xv.data_ptr() == x.data_ptr() and xbs == (2 if case.sliced and B > 1 else 1) * C * HW      # (one sample: no batch stride)
    gxd = gx.to(DEV)
    PAD, SENT = 64, 12345.0
    outs = []
    for _ in range(2):
        buf = torch.full((B * C * HW + 2 * PAD,), SENT, device=DEV)
        gz = buf[PAD: PAD + B * C * HW].view(B, C, H, H)
        _hip.call("cf_flow_step_inv_bwd_data", P(xv), P(gxd), P(ws), P(wsb), P(wsv), P(gz), B, C, H, H, xbs, st)
        torch.cuda.synchronize()
        assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + B * C * HW:] == SENT).all())
        outs.append(gz)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    err, b = R.rel_err(outs[0], want), R.bar(floor)
    print("inv_bwd %s form=%s: err %.3e floor %.3e bar %.3e" % (case.id, os.environ.get("CONTEXTFLOW_DIRECT_CONV", "0"), err, floor, b))
    assert err <= b, "%s: err %.3e > bar %.3e (floor %.3e)" % (case.id, err, b, floor)
    _hip.call("cf_flow_step_inv_bwd_data", None, None, None, None, None, None, 0, C, H, H, C * HW, st)      # B == 0: a no-op


@pytest.mark.gpu
def test_step_inv_bwd_data_in_a_child_process_with_the_direct_form():
    """4, once more in ONE fresh child with CONTEXTFLOW_DIRECT_CONV=1 (read once per process)."""
    env = dict(os.environ, CONTEXTFLOW_DIRECT_CONV="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_decode_grad.py"), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           "-k", "test_step_inv_bwd_data_per_geometry"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if "inv_bwd " in ln and " form=1:" in ln]
    print("\n".join(lines))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert len(lines) == len(U.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4-bytes-off"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n_keep,aug_n", [(3072, 1024), (1024, 0), (7, 5)])
def test_postprocess_inv_bwd(L, n_keep, aug_n, B, off):
    """5. cf_postprocess_inv_bwd against fp64 autograd through the oracle's pre-processing inverse without the floor (sigmoid,
    affine_inv x 2): 1e-6 of scale; the Augment gradient exactly zero; batch-strided y, sentinels around gy."""
    from contextflow_amd.layers import _hip
    g = torch.Generator().manual_seed(n_keep + 7 * B + off)
    n = n_keep + aug_n
    y = 3.0 * torch.randn(B, n, generator=g)
    gx = torch.randn(B, n_keep, generator=g)
    y64 = y[:, :n_keep].double().requires_grad_(True)
    x64 = fo.affine_inv(fo.affine_inv(torch.sigmoid(y64), fo.ALPHA, 1 / (1 - 2 * fo.ALPHA)), 0.0, 256.0)
    (x64 * gx.double()).sum().backward()
    ref = y64.grad
    ybs = n + 4
    ybuf = torch.zeros(B * ybs + off + 4, device=DEV)
    yd = ybuf[off: off + B * ybs].view(B, ybs)
    yd[:, :n] = y.to(DEV)
    gxbuf = torch.zeros(B * n_keep + off, device=DEV)
    gxd = gxbuf[off:].view(B, n_keep)
    gxd.copy_(gx.to(DEV))
    PAD, SENT = 8, 12345.0
    buf = torch.full((B * n + 2 * PAD + off,), SENT, device=DEV)
    gy = buf[PAD + off: PAD + off + B * n].view(B, n)
    s12 = 256.0 * S2_32
    _hip.call("cf_postprocess_inv_bwd", _hip.p(yd), _hip.p(gxd), _hip.p(gy), B, n_keep, aug_n, ybs, n, s12, _hip.stream())
    torch.cuda.synchronize()
    assert bool((buf[:PAD + off] == SENT).all()) and bool((buf[PAD + off + B * n:] == SENT).all())
    scale = max(1.0, ref.abs().max().item())
    err = (gy[:, :n_keep].cpu().double() - ref).abs().max().item() / scale
    print("postprocess_inv_bwd n_keep=%d aug=%d B=%d off=%d: %.2e of scale %.1f (bar 1e-06)" % (n_keep, aug_n, B, off, err, scale))
    assert err <= 1e-6
    assert bool((gy[:, n_keep:] == 0).all())


@pytest.mark.gpu
def test_layer_path_coupling_rule(L):
    """6. A Coupling with a 1x1 kernel (not fusable) at (6, 5, 3), B = 3: `inverse(differentiable=True)` + backward against fp64
    autograd through the oracle's coupling_inv, bar(fp32 CPU floor)."""
    import contextflow_amd as cfa
    C, H, W, B = 6, 5, 3, 3
    torch.manual_seed(3)
    cpl = L.Coupling(C, kernel_size=(1, 1), padding=(0, 0))
    flow = cfa.layers.FlowSequential(L.GaussianMixtureDistribution(size=(C, H, W), mixtures=2, components=8), cpl).to(DEV)
    g = torch.Generator().manual_seed(4)
    z, gx = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)

    def oracle(dtype):
        p = {"0." + k: v.detach().cpu().to(dtype) for k, v in cpl.state_dict().items()}
        zz = z.to(dtype).clone().requires_grad_(True)
        x = fo.coupling_inv(zz, p, "0.", (0, 0))
        (x * gx.to(dtype)).sum().backward()
        return x.detach(), zz.grad
    x64, ref = oracle(torch.float64)
    floor = R.rel_err(oracle(torch.float32)[1], ref)
    zd = z.to(DEV).requires_grad_(True)
    x = flow.inverse(zd, differentiable=True)
    assert x.grad_fn is not None
    (x * gx.to(DEV)).sum().backward()
    assert R.rel_err(x, x64) < 1e-5
    err, b = R.rel_err(zd.grad, ref), R.bar(floor)
    print("layer-path coupling VJP: err %.3e floor %.3e bar %.3e" % (err, floor, b))
    assert err <= b
    assert all(p.grad is None for p in flow.parameters())


def _recording(monkeypatch):
    from contextflow_amd.layers import _hip
    names, real = [], _hip.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_hip, "call", recording)
    return names


NSTEPS = {"cifar10": 12, "mnist": 4}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mnist", "cifar10"])
def test_whole_chain_against_fp64_autograd(L, name, monkeypatch):
    """7. decode(trace latents, differentiable=True) + backward under a fixed random gx against fp64 autograd through
    fo.flow_inverse stopped in front of the dequantisation.  Error = max|got - ref| / max|ref| for z and every half; bar =
    max(1e-4, 3 x the fp32 CPU floor of the same graph).  The forward value within 1e-5 of scale of the trace's continuous
    input; one cf_flow_step_inv_bwd_data per fused step and no weight-gradient work.
    Measured on an MI355X, error (fp32 floor of that machine's CPU): mnist z 4.0e-7 (4.9e-7); cifar10 z 6.0e-7 (1.5e-6), halves
    5.1e-7 (1.3e-6) and 5.8e-7 (1.1e-6); forward 4.2e-7 / 6.9e-7 of scale 256."""
    from tests.gpu_util import build_model
    ops, params, _, _, inputs, _, _, _ = problem(name)
    z, halves, gx, x64, ref, floor = U.chain_reference(name)
    model = build_model(name, params)
    lat = [h.float().to(DEV).requires_grad_(True) for h in halves] + [z.float().to(DEV).requires_grad_(True)]
    names = _recording(monkeypatch)
    x = model.decode(lat, differentiable=True)
    assert x.grad_fn is not None and tuple(x.shape) == tuple(x64.shape)
    (x * gx.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    cont = inputs[1]                                          # x + u: what entered the first Normalization
    scale = max(1.0, cont.abs().max().item())
    fwd = (x.detach().cpu().double() - cont).abs().max().item() / scale
    print("decode_grad %s forward: %.2e of scale %.1f (bar 1e-05)" % (name, fwd, scale))
    assert fwd <= 1e-5
    assert names.count("cf_flow_step_inv_bwd_data") == NSTEPS[name] == names.count("cf_flow_step_inv")
    assert names.count("cf_postprocess_inv_bwd") == 1
    assert not [n for n in names if n.startswith("cf_wgrad") or n.startswith("cf_step_wgrads") or n == "cf_flow_step_bwd_taped"
                or "param_grads" in n], names
    assert all(p.grad is None for p in model.parameters())
    failed = []
    for what, t, r, fl in zip(["half%d" % i for i in range(len(halves))] + ["z"], lat, ref[1:] + ref[:1], floor[1:] + floor[:1]):
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.is_contiguous()
        err = (t.grad.cpu().double() - r).abs().max().item() / r.abs().max().item()
        bar = max(1e-4, 3.0 * fl)
        print("decode_grad %s %s: relative error %.3e, fp32 floor %.3e, bar %.3e" % (name, what, err, fl, bar))
        if not err < bar:
            failed.append((what, err, bar))
    assert not failed, failed


@pytest.mark.gpu
def test_default_flag_is_the_plain_walk(L, monkeypatch):
    """8a. differentiable=False with a latent that requires a gradient: no grad_fn, bit for bit the call on the detached latent;
    the launch list of a plain decode holds one cf_flow_step_inv per step, one cf_postprocess_inv and none of the new symbols."""
    from tests.gpu_util import build_model
    ops, params, z, halves, _, _, _, _ = problem("mnist")
    model = build_model("mnist", params)
    lat = [h.float().to(DEV) for h in halves] + [z.float().to(DEV)]
    model.decode(lat)                                         # (the first call also packs the steps' tables)
    names = _recording(monkeypatch)
    x0 = model.decode(lat)
    n0 = list(names)
    del names[:]
    x1 = model.decode([t.clone().requires_grad_(True) for t in lat], differentiable=False)
    n1 = list(names)
    monkeypatch.undo()
    assert x1.grad_fn is None and not x1.requires_grad and torch.equal(x0, x1)
    assert n0 == n1 and n0.count("cf_flow_step_inv") == NSTEPS["mnist"] and n0.count("cf_postprocess_inv") == 1
    assert not set(n0) & set(NEW_SYMBOLS)
    zi = torch.randn(3, *z.shape[1:], generator=torch.Generator().manual_seed(1)).to(DEV)
    torch.manual_seed(5); a = model.inverse(zi)
    torch.manual_seed(5); b = model.inverse(zi.clone().requires_grad_(True))
    assert b.grad_fn is None and torch.equal(a, b)
    # without a latent that requires a gradient, and under no_grad: the continuous result, detached
    xc = model.decode(lat, differentiable=True)
    with torch.no_grad():
        xn = model.decode([t.clone().requires_grad_(True) for t in lat], differentiable=True)
    assert xc.grad_fn is None and xn.grad_fn is None and torch.equal(xc, xn)
    assert bool((xc.floor() - x0).abs().max() <= 1.0) and bool(((xc.floor() - x0) != 0).float().mean() < 1e-3)


@pytest.mark.gpu
def test_central_difference_spot_check(L):
    """8b. A smoke check, not a bar on accuracy: on mnist at B = 2 a central difference in fp32 along two random directions over
    all latents agrees with the VJP to 2 %."""
    from tests.gpu_util import build_model
    ops, params, z, halves, _, _, _, _ = problem("mnist")
    model = build_model("mnist", params)
    lat0 = [h[:2].float().to(DEV) for h in halves] + [z[:2].float().to(DEV)]
    g = torch.Generator().manual_seed(9)
    lat = [t.clone().requires_grad_(True) for t in lat0]
    x = model.decode(lat, differentiable=True)
    gx = torch.randn(x.shape, generator=g).to(DEV)
    (x * gx).sum().backward()
    f = lambda ts: float((model.decode(ts, differentiable=True).double() * gx.double()).sum())
    # step: the map is piecewise smooth - every ReLU unit whose pre-activation changes sign between z - h d and z + h d adds a
    # share of its slope change, so the difference's error falls like h (not h^2) until the fp32 rounding of the two forward runs,
    # ~4e-3 / (2 h) on derivatives of 5e2 .. 5e3, takes over: 2e-4 balances the two well inside the 2 %
    h = 2e-4
    for k in range(2):
        dirs = [torch.randn(t.shape, generator=g).to(DEV) for t in lat0]
        fd = (f([t + h * d for t, d in zip(lat0, dirs)]) - f([t - h * d for t, d in zip(lat0, dirs)])) / (2 * h)
        an = sum(float((t.grad.double() * d.double()).sum()) for t, d in zip(lat, dirs))
        print("central difference %d: %.6e against the VJP's %.6e (%.2e relative)" % (k, fd, an, abs(fd - an) / abs(an)))
        assert abs(fd - an) <= 0.02 * abs(an)


@pytest.mark.gpu
def test_refusals_empty_batch_and_the_lone_conv1x1(L):
    """8c. Every refusal names what it refuses; an empty batch; backward of a lone Conv1x1 is W^-T g."""
    import contextflow_amd as cfa
    from tests.gpu_util import build_model
    ops, params, z, halves, _, _, _, _ = problem("mnist")
    model = build_model("mnist", params)
    lat = [h.float().to(DEV) for h in halves] + [z.float().to(DEV)]
    with pytest.raises(ValueError, match="clamp"):
        model.decode(lat, clamp=True, differentiable=True)
    with pytest.raises(NotImplementedError, match="return_logp"):
        model.decode(lat, return_logp=True, differentiable=True)
    with pytest.raises(NotImplementedError, match="return_logp"):
        model.inverse(lat[-1], return_logp=True, differentiable=True)
    with pytest.raises(NotImplementedError, match="context"):
        model.inverse(lat[-1], context=torch.zeros(lat[-1].shape[0], 1, device=DEV), differentiable=True)
    size = (4, 2, 2)
    dist = L.GaussianMixtureDistribution(size=size, mixtures=2, components=4)
    zz = torch.randn(3, *size, generator=torch.Generator().manual_seed(2)).to(DEV)
    for layer, word in ((L.LeakyRelu(0.1), "LeakyRelu"), (L.Augment(L.StandardNormal((4, 2, 1)), 1, split_dim=3), "Augment")):
        flow = cfa.layers.FlowSequential(dist, L.Conv1x1(size), layer).to(DEV)
        with pytest.raises(NotImplementedError, match=word):
            flow.inverse(zz if word != "Augment" else torch.randn(3, 4, 2, 3, device=DEV), differentiable=True)
    # an empty batch
    e = [t[:0].clone().requires_grad_(True) for t in lat]
    xe = model.decode(e, differentiable=True)
    assert xe.shape[0] == 0 and xe.grad_fn is not None
    xe.sum().backward()
    assert all(t.grad is not None and t.grad.shape == t.shape for t in e)
    # a lone Conv1x1: x = W^-1 z, so dL/dz = W^-T g
    conv = L.Conv1x1(size)
    with torch.no_grad():
        conv.NN.add_(0.2 * torch.randn(4, 4, generator=torch.Generator().manual_seed(3)))
    flow = cfa.layers.FlowSequential(dist, conv).to(DEV)
    zr = zz.clone().requires_grad_(True)
    gx = torch.randn(3, *size, generator=torch.Generator().manual_seed(4)).to(DEV)
    x = flow.inverse(zr, differentiable=True)
    (x * gx).sum().backward()
    Winv = torch.linalg.inv(conv.NN.detach().double().cpu())
    want = torch.einsum("oi,bohw->bihw", Winv, gx.double().cpu())
    assert R.rel_err(zr.grad, want) < 1e-5
    assert R.rel_err(x, torch.einsum("oi,bihw->bohw", Winv, zz.double().cpu())) < 1e-5
