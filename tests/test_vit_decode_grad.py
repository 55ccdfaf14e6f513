"""`inverse` / `decode` with differentiable=True on the transformer flows: the latent gradient of their backward walk.

CPU: the reference of the inverse transformer step's vector-Jacobian product (tests/vit_decode_grad_util.py::vit_step_inv_ref)
against the forward reference with no kernel involved (J_F^T J_F^-T = I); the ABI.  GPU: cf_vit_inv_step_bwd_data alone through the
C ABI; the committed smap fixture per step, over two four-step sub-chains and as a whole against fp64 autograd through
fo.flow_inverse, on the kernel route and on the layer rule; a geometry outside the kernel; the empty batch; what keeps raising.

The accuracy claim is carried by the per-step and four-step checks: the eight-step chain amplifies by about 7e3, fp32 CPU autograd
is itself 1e-3 .. 3e-3 from fp64 there, and the whole-model check is held at three times that floor."""
import os

import pytest
import torch

from tests import vit_decode_grad_util as U
from tests import vit_step_fp64_ref as V
from tests.sample_logp_util import problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NEW_SYMBOLS = ("cf_vit_inv_step_bwd_ws_bytes", "cf_vit_inv_step_bwd_prepare", "cf_vit_inv_step_bwd_data")
ids = lambda cases: ["B%d-d%d%s" % (c.B, c.depth, "-slice" if c.sliced else "") for c in cases]


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", U.CASES, ids=ids(U.CASES))
def test_vit_step_inv_ref_inverts_the_forward_reference(case):
    """1. gz = VJP_inv(gx) by autograd through vit_step_inv_ref at z = step_ref(x); then step_ref's gx under upstream gz with gld = 0
    returns the drawn gx (J_F^T J_F^-T = I): 1e-10 relative, fp64, no kernel involved.  x is recovered to 1e-12 on the way."""
    d, ref = U.drawn(case)
    inv = U.vit_step_inv_ref(d, case.depth, ref["z"], gx=d["gz"])
    assert V.rel_err(inv["x"], d["x"].double()) < 1e-12
    back = V.step_ref(dict(d, gz=inv["gz"], gld=torch.zeros_like(d["gld"])), case.depth)
    err = V.rel_err(back["gx"], d["gz"].double())
    print("%s: J_F^T J_F^-T gx against gx, fp64: %.2e relative" % (case.id, err))
    assert err < 1e-10


def test_abi_of_the_new_entry_points():
    """2. Declared in the header, present in _hip's signature table, exported by the built library; the ABI version stays."""
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
    assert _hip.lib().cf_vit_inv_step_bwd_ws_bytes(26) >= 4 * 26 * 26
    for C in (25, 38, 55, 6):
        assert _hip.lib().cf_vit_inv_step_bwd_ws_bytes(C) == 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


def _step_modules(L, p, depth):
    conv, act, cpl = L.Conv1x1(V.SZ), L.ActNorm(V.SZ), L.TransCoupling(V.SZ, V.PATCH)
    vit = cpl.NN[0]
    vit.transformer.layers = vit.transformer.layers[:depth]               # before anything is packed
    own = dict(cpl.named_parameters())
    assert sorted(own) == sorted(V.vit_names(depth))
    with torch.no_grad():
        for k, v in own.items():
            v.copy_(p[k])
        conv.NN.copy_(p["Conv1x1.NN"]); act.NN_t.copy_(p["ActNorm.NN_t"]); act.NN_logs.copy_(p["ActNorm.NN_logs"]); act.initialized.fill_(1)
    act._init_done = True
    return conv.to(DEV), act.to(DEV), cpl.to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("case", U.CASES, ids=ids(U.CASES))
def test_vit_step_inv_bwd_data(L, case):
    """3. cf_vit_inv_step_bwd_data at the exact step input x (dense, and a channel slice of a wider tensor) under the drawn gx,
    against fp64 autograd through vit_step_inv_ref: bar = min(1e-4, max(2e-6, 4 x floor)) of the largest entry, floor = the error
    of fp32 CPU autograd on the same graph, itself <= 2e-5 (the cap is never what passes the test).  gz pre-filled with NaN and
    framed by sentinels; two launches the same bits; B == 0 returns without touching gz.
    Measured on an MI355X: 1.7e-7 .. 3.3e-7 against floors of 2.6e-7 .. 5.9e-7 (profiles/vit_decode_grad.md)."""
    from contextflow_amd.layers import _hip
    lib, P, st = _hip.lib(), _hip.p, _hip.stream()
    d, ref = U.drawn(case)
    B, depth, C, HW = case.B, case.depth, V.C, V.HW
    gx = d["gz"]
    want = U.vit_step_inv_ref(d, depth, ref["z"], gx=gx)["gz"]
    floor = U.vit_step_inv_floor(d, depth, ref["z"], gx, want)
    conv, act, cpl = _step_modules(L, d["p"], depth)
    t = L.TransCoupling.step_tables([(cpl, conv.NN, act.NN_t, act.NN_logs)], torch.device(DEV), "rs", winv=True, bwd=True)[0]
    wsv = torch.empty(lib.cf_vit_inv_step_bwd_ws_bytes(C), device=DEV, dtype=torch.uint8)
    _hip.call("cf_vit_inv_step_bwd_prepare", P(t.winv), P(_hip.f32(act.NN_logs.detach())), P(wsv), C, st)
    x = d["big"].to(DEV)[:, :C] if d["big"] is not None else d["x"].to(DEV)
    xv, xbs = _hip.bview(x)
    assert xv.data_ptr() == x.data_ptr() and xbs == (2 if case.sliced else 1) * C * HW
    gxd = gx.to(DEV)
    PAD, SENT = 64, 12345.0
    outs = []
    for _ in range(2):
        buf = torch.full((B * C * HW + 2 * PAD,), SENT, device=DEV)
        gz = buf[PAD: PAD + B * C * HW].view(B, C, HW, 1)
        gz.fill_(float("nan"))
        _hip.call("cf_vit_inv_step_bwd_data", P(xv), P(gxd), P(t.ws), P(t.wsb), P(wsv), P(gz), B, C, depth, xbs, st)
        torch.cuda.synchronize()
        assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + B * C * HW:] == SENT).all())
        outs.append(gz)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    err, b = V.rel_err(outs[0], want), V.bar(floor)
    print("vit_inv_bwd B%d d%d%s: err %.3e floor %.3e bar %.3e" % (B, depth, " slice" if case.sliced else "", err, floor, b))
    assert floor <= 2e-5
    assert err <= b, "%s: err %.3e > bar %.3e (floor %.3e)" % (case.id, err, b, floor)
    keep = torch.full((C * HW,), SENT, device=DEV)
    _hip.call("cf_vit_inv_step_bwd_data", P(xv), P(gxd), P(t.ws), P(t.wsb), P(wsv), P(keep), 0, C, depth, xbs, st)      # B == 0: a no-op
    _hip.call("cf_vit_inv_step_bwd_data", None, None, None, None, None, None, 0, C, depth, C * HW, st)
    torch.cuda.synchronize()
    assert bool((keep == SENT).all())


@pytest.mark.gpu
def test_vit_step_inv_bwd_data_refuses_other_geometries(L):
    """3b. Another channel count or a depth past the kernel's LDS budget: CF_ERR_UNSUPPORTED, by name."""
    from contextflow_amd.layers import _hip
    lib = _hip.lib()
    q = torch.zeros(64, device=DEV).data_ptr()
    for C, depth in ((38, 6), (26, 7), (26, 0)):
        rc = lib.cf_vit_inv_step_bwd_data(q, q, q, q, q, q, 4, C, depth, C * 8, None)
        assert rc == -2 and b"cf_vit_inv_step_bwd_data" in lib.cf_last_error(), (C, depth, rc)
    assert lib.cf_vit_inv_step_bwd_prepare(q, q, q, 38, None) == -2


def _recording(monkeypatch):
    from contextflow_amd.layers import _hip
    names, real = [], _hip.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_hip, "call", recording)
    return names


@pytest.fixture(scope="module")
def smap(L):
    from tests.gpu_util import build_model
    return build_model("smap", problem("smap")[1])


def _sub_flow(L, model, lo, hi):
    import contextflow_amd as cfa
    return cfa.layers.FlowSequential(model.dist, *model.sequence_modules[lo:hi])


def _walk_grad(flow, z, gx, what="inverse"):
    zd = z.float().to(DEV).requires_grad_(True)
    x = flow.inverse(zd, differentiable=True) if what == "inverse" else flow.decode([zd], differentiable=True)
    assert x.grad_fn is not None
    x.backward(gx.float().to(DEV))
    torch.cuda.synchronize()
    assert zd.grad is not None and zd.grad.shape == zd.shape and zd.grad.is_contiguous()
    return x.detach(), zd.grad


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["kernel", "layers"])
@pytest.mark.parametrize("k", range(U.NSTEPS))
def test_smap_each_step(L, smap, k, route, monkeypatch):
    """4. Each of the fixture's eight steps as FlowSequential(dist, conv, act, cpl) of the model's own modules, from the traced step
    output, against fp64 autograd through fo.flow_inverse under a randn upstream (seed 3): bar max(2e-6, 4 x floor), floor (fp32
    CPU autograd on the same graph) <= 2e-6.  route "kernel": one cf_vit_inv_step_bwd_data launch; "layers": the same modules with
    fused = False on the coupling take the InvTransCoupling / InvAct / InvConv rules, and meet the same bar."""
    z, gx, x64, ref, floor = U.smap_step(k)
    flow = _sub_flow(L, smap, 1 + 3 * k, 4 + 3 * k)
    cpl = flow.sequence_modules[2]
    names = _recording(monkeypatch)
    try:
        cpl.fused = route == "kernel"
        x, g = _walk_grad(flow, z, gx)
    finally:
        cpl.fused = True
    monkeypatch.undo()
    assert names.count("cf_vit_inv_step_bwd_data") == (1 if route == "kernel" else 0)
    assert not [n for n in names if "wgrad" in n or "param_grads" in n], names
    assert all(p.grad is None for p in flow.parameters())
    assert U.rel(x, x64) < 1e-5
    err, bar = U.rel(g, ref), max(2e-6, 4.0 * floor)
    print("vit decode_grad smap step %d %s: err %.3e floor %.3e bar %.3e" % (k, route, err, floor, bar))
    assert floor <= 2e-6
    assert err <= bar


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(U.SUBCHAINS))
def test_smap_four_step_sub_chains(L, smap, name):
    """5. Steps 1 - 4 (ops[1:13]) and 5 - 8 (ops[13:25]) from the traced output of the last of them: bar max(1e-4, 3 x floor),
    floor <= 3e-5."""
    lo, hi = U.SUBCHAINS[name]
    z, gx, x64, ref, floor = U.smap_range(lo, hi)
    x, g = _walk_grad(_sub_flow(L, smap, lo, hi), z, gx)
    err, bar = U.rel(g, ref), max(1e-4, 3.0 * floor)
    print("vit decode_grad smap %s: err %.3e floor %.3e bar %.3e" % (name, err, floor, bar))
    assert floor <= 3e-5
    assert err <= bar


@pytest.mark.gpu
def test_smap_whole_model(L, smap, monkeypatch):
    """6. decode([z], differentiable=True) + backward(g) on the whole fixture against fp64 autograd through fo.flow_inverse: held at
    3 x the fp32 CPU floor of the same graph (computed here, <= 1e-2: the chain amplifies by about 7e3); one
    cf_vit_inv_step_bwd_data per step and no weight-gradient work; the forward value is model.inverse(z) bit for bit; a latent
    without requires_grad, or a call under no_grad, returns the same values detached."""
    z, gx, x64, ref, floor = U.smap_whole()
    zd = z.float().to(DEV)
    plain = smap.inverse(zd)
    names = _recording(monkeypatch)
    x, g = _walk_grad(smap, z, gx, "decode")
    monkeypatch.undo()
    assert names.count("cf_vit_inv_step_bwd_data") == U.NSTEPS
    assert not [n for n in names if "wgrad" in n or "param_grads" in n or n == "cf_vit_step_bwd"], names
    assert all(p.grad is None for p in smap.parameters())
    assert tuple(x.shape) == tuple(x64.shape) and torch.equal(x, plain)
    xi = smap.inverse(zd.clone().requires_grad_(True), differentiable=True)
    assert xi.grad_fn is not None and torch.equal(xi.detach(), plain)
    xc = smap.decode([zd], differentiable=True)
    with torch.no_grad():
        xn = smap.decode([zd.clone().requires_grad_(True)], differentiable=True)
    assert xc.grad_fn is None and not xc.requires_grad and xn.grad_fn is None and torch.equal(xc, plain) and torch.equal(xn, plain)
    err, bar = U.rel(g, ref), 3.0 * floor
    print("vit decode_grad smap whole: err %.3e floor %.3e bar %.3e; forward %.3e of fp64" % (err, floor, bar, U.rel(x, x64)))
    assert floor <= 1e-2
    assert err <= bar


@pytest.mark.gpu
def test_default_flag_launches_nothing_new(L, smap, monkeypatch):
    """6b. differentiable=False: the plain walk's launch list, none of the new symbols, no grad_fn."""
    zd = problem("smap")[2].float().to(DEV)
    smap.decode([zd])
    names = _recording(monkeypatch)
    x0 = smap.decode([zd])
    n0 = list(names)
    del names[:]
    x1 = smap.decode([zd.clone().requires_grad_(True)], differentiable=False)
    n1 = list(names)
    monkeypatch.undo()
    assert n0 == n1 and n0.count("cf_vit_coupling") == U.NSTEPS and not set(n0) & set(NEW_SYMBOLS)
    assert x1.grad_fn is None and torch.equal(x0, x1)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [6, 38, 56])
def test_geometry_outside_the_kernel(L, C):
    """7. Conv1x1 -> ActNorm -> TransCoupling((C, 8, 1), (2, 1)), B = 3, at C = 6 and at the channel counts of the smd and (behind
    its Augment) msl flows: the layer rule, against fp64 autograd through the oracle's ops: bar max(1e-4, 3 x floor), floor <= 3e-5."""
    import contextflow_amd as cfa
    sz, patch, B = (C, 8, 1), (2, 1), 3
    torch.manual_seed(11)
    conv, act, cpl = L.Conv1x1(sz), L.ActNorm(sz), L.TransCoupling(sz, patch)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        conv.NN.add_(0.1 * torch.randn(C, C, generator=g))
        act.NN_t.copy_(0.3 * torch.randn(C, generator=g).view_as(act.NN_t))
        act.NN_logs.copy_(0.4 * torch.randn(C, generator=g).view_as(act.NN_logs))
        act.initialized.fill_(1)
    act._init_done = True
    flow = cfa.layers.FlowSequential(L.GaussianMixtureDistribution(size=sz, mixtures=1, components=4), conv, act, cpl).to(DEV)
    ops = [("conv1x1", 0, sz), ("actnorm", 1, sz), ("transcoupling", 2, sz, patch)]
    params = {"%d.%s" % (i, k): v.detach().cpu() for i, m in enumerate((conv, act, cpl)) for k, v in m.state_dict().items()}
    z = torch.randn(B, *sz, generator=g)
    gx, x64, ref, floor = U.inverse_reference(ops, params, z)
    assert not cpl.step_supported(sz)
    x, got = _walk_grad(flow, z, gx)
    assert U.rel(x, x64) < 1e-5
    err, bar = U.rel(got, ref), max(1e-4, 3.0 * floor)
    print("vit decode_grad (%d, 8, 1): err %.3e floor %.3e bar %.3e" % (C, err, floor, bar))
    assert floor <= 3e-5
    assert err <= bar
    assert all(p.grad is None for p in flow.parameters())


@pytest.mark.gpu
def test_empty_batch_and_what_keeps_raising(L, smap):
    """8. An empty batch has a grad_fn and a gradient of the latent's shape; clamp=True: ValueError; return_logp=True:
    NotImplementedError; a smap specialist's TransCoupling with a context net: NotImplementedError naming the layer and its index."""
    import contextflow_amd as cfa
    zd = problem("smap")[2].float().to(DEV)
    e = zd[:0].clone().requires_grad_(True)
    xe = smap.decode([e], differentiable=True)
    assert xe.shape[0] == 0 and xe.grad_fn is not None
    xe.sum().backward()
    assert e.grad is not None and e.grad.shape == e.shape
    with pytest.raises(ValueError, match="clamp"):
        smap.decode([zd], clamp=True, differentiable=True)
    with pytest.raises(NotImplementedError, match="return_logp"):
        smap.decode([zd], return_logp=True, differentiable=True)
    with pytest.raises(NotImplementedError, match="return_logp"):
        smap.inverse(zd, return_logp=True, differentiable=True)
    cfg, ds, MM = cfa.preset_config("smap", coupling="trans")
    cfg.update(generalist=False, contextflow=True)
    torch.manual_seed(1)
    flow = cfa.create_model(cfg, ds, MM, contexts=[3]).to(DEV).eval()
    zz = torch.randn(2, *flow.dist.mG.shape[2:], generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"TransCoupling with a context net \(layer \d+\)"):
        flow.decode([zz], torch.zeros(2, 1, dtype=torch.long, device=DEV), differentiable=True)
