"""`inverse` / `decode` of a specialist flow with differentiable=True: the latent gradient of the backward walk under a context
(DESIGN 7.3g).

CPU: the fp64 reference and the fp32 floor of the whole chain (tests/specialist_decode_grad_util.py::chain_reference), the ReLU band
of every kernel case, the adjoint identity of the restated inverse coupling.  GPU: the ABI, the three new kernels alone -
cf_flow_step_inv_ctx, cf_flow_step_inv_bwd_ctx_data, cf_affine_ctx_inv_bwd_data - the whole walk of the chain fixtures against fp64
autograd, the pixels, and the semantics of the flag."""
import os

import pytest
import torch

from tests import specialist_decode_grad_util as U
from tests import specialist_inverse_util as SU
from tests import step_fp64_ref as R
from tests.test_specialist_inverse import SHAPES, _operands

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = SU.DEV
NEW_SYMBOLS = ("cf_flow_step_inv_ctx", "cf_flow_step_inv_bwd_ctx_data", "cf_affine_ctx_inv_bwd_data")
ids = lambda cases: [c.id for c in cases]


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fxname", U.GRAD_FIXTURES + ["mnist_eye_cf"])
def test_fp64_reference_and_fp32_floor_of_the_chain(fxname):
    """1. fp64 autograd through spec_inverse continued through the pre-processing (stopped in front of the floor), upstream seed 5,
    B = 4, and what fp32 CPU autograd loses on the same graph.  On the six fixtures of the gradient comparison every floor is
    finite and below 1e-4 (measured: 4.9e-7 .. 7.9e-6; forward value 8.0e-7 .. 9.6e-6 of scale 256); mnist_eye_cf, whose fp32
    gradient is 6.7e-4 from fp64, is shown and kept out of that comparison."""
    gx, x64, ref, floor, fwd = U.chain_reference(fxname)
    p = SU.problem(fxname, 4)
    assert len(ref) == len(floor) == 1 + len(p.halves) and tuple(x64.shape) == tuple(p.x.shape)
    assert SU.err_of(x64, p.inputs[1]) < 1e-9                    # the restatement returns the trace's continuous input x + u
    print("%s: gradient floors %s, forward %.1e" % (fxname, ", ".join("%.1e" % f for f in floor), fwd))
    assert all(torch.isfinite(r).all() for r in ref)
    if fxname in U.GRAD_FIXTURES:
        assert all(0.0 <= f < 1e-4 for f in floor) and fwd < 1e-4


@pytest.mark.parametrize("case", U.BWD_CASES, ids=ids(U.BWD_CASES))
def test_kernel_inputs_stay_clear_of_the_relu_band(case):
    """2. The VJP kernel's masks cannot be read back: the fp64 run of every case has NO unit inside step_fp64_ref.in_band."""
    _, ref = U.drawn(case)
    assert R.band_share(ref)[3] == 0, "%s: units inside the band - pick another seed" % case.id


@pytest.mark.parametrize("case", U.BWD_CASES[::4] + U.BWD_CASES[2::4], ids=ids(U.BWD_CASES[::4] + U.BWD_CASES[2::4]))
def test_coupling_inv_ref_inverts_the_forward_reference(case):
    """3. gz = VJP_inv(gx) by autograd through coupling_inv_ref at z = step_ref(x); then the forward coupling's gx under upstream gz
    with gld = 0 returns the drawn gx (J_F^T J_F^-T = I): 1e-10 relative, fp64, both bias modes, no kernel involved."""
    d, ref = U.drawn(case)
    inv = U.coupling_inv_ref(d, ref["z"], case.mode, gx=d["gz"])
    assert R.rel_err(inv["x"], d["x"].double()) < 1e-12
    back = R.step_ref(dict(d, gz=inv["gz"], gld=torch.zeros_like(d["gld"])), mode=case.mode)
    err = R.rel_err(back["gx"], d["gz"].double())
    print("%s: J_F^T J_F^-T gx against gx, fp64: %.2e relative" % (case.id, err))
    assert err < 1e-10


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


@pytest.mark.gpu
def test_abi_of_the_new_entry_points(L):
    """4. Declared in the header, present in _hip's signature table, exported by the built library; the ABI version stays 16."""
    import ctypes
    import re
    from contextflow_amd import build
    from contextflow_amd.layers import _hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "contextflow_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.build())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, src), s
        assert s in _hip.SIGNATURES and hasattr(lib, s), s
    assert "#define CF_ABI_VERSION 16" in src and _hip.ABI_VERSION == 16 and _hip.lib().cf_abi_version() == 16


def _coupling_tables(case, p, bwd=False):
    """(ws [, wsb]) of the coupling of a case: the identity-front tables of cf_flow_step_prepare / cf_flow_step_bwd_prepare."""
    from contextflow_amd.layers import _hip
    lib, P, st = _hip.lib(), _hip.p, _hip.stream()
    C, H = case.C, case.H
    w = {k: v.to(DEV).contiguous() for k, v in p.items()}
    eye, zero = torch.eye(C, device=DEV), torch.zeros(C, device=DEV)
    ws = torch.empty(lib.cf_flow_step_ws_bytes(C, H, H), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_prepare", P(eye), P(zero), P(zero), P(w["NN.0.weight"]), P(w["NN.0.bias"]), P(w["NN.2.weight"]),
              P(w["NN.2.bias"]), P(w["NN.4.weight"]), P(w["NN.4.bias"]), P(ws), C, H, H, st)
    if not bwd:
        return ws
    wsb = torch.empty(lib.cf_flow_step_bwd_ws_bytes(C, H, H), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_bwd_prepare", P(eye), P(zero), P(w["NN.0.weight"]), P(w["NN.2.weight"]), P(w["NN.4.weight"]), P(wsb), C, H, H, st)
    return ws, wsb


@pytest.mark.gpu
@pytest.mark.parametrize("case", U.FWD_CASES, ids=ids(U.FWD_CASES))
def test_flow_step_inv_ctx_per_geometry(L, case):
    """5. cf_flow_step_inv_ctx at the exact z of the fp64 forward coupling (dense, and a channel slice of a tensor twice as wide):
    the coupling input back to 1e-5 of max(1, max|ref|), the inverse step's bar in tests/test_sampling.py; both bias modes; B in
    {1, 37}; the sentinels framing x intact; B = 0 a no-op.
    Measured on an MI355X: 1.2e-7 .. 9.5e-7 of scale (profiles/specialist_decode_grad.md)."""
    from contextflow_amd.layers import _hip
    P, st = _hip.p, _hip.stream()
    d, ref = U.drawn(case)
    B, C, H = case.B, case.C, case.H
    n = C * H * H
    want = U.coupling_inv_ref(d, ref["z"], case.mode)["x"]
    assert R.rel_err(want, d["x"].double()) < 1e-12
    ws = _coupling_tables(case, d["p"])
    z32 = ref["z"].float()
    if case.sliced:
        z = torch.cat([z32, torch.randn(B, C, H, H, generator=torch.Generator().manual_seed(1))], 1).to(DEV)[:, :C]
    else:
        z = z32.to(DEV)
    zv, zbs = _hip.bview(z)
    assert zbs == (2 if case.sliced and B > 1 else 1) * n
    PAD, SENT = 64, 12345.0
    buf = torch.full((B * n + 2 * PAD,), SENT, device=DEV)
    x = buf[PAD: PAD + B * n].view(B, C, H, H)
    _hip.call("cf_flow_step_inv_ctx", P(zv), P(x), P(ws), P(d["sbias"].to(DEV)), case.mode, B, C, H, H, zbs, st)
    torch.cuda.synchronize()
    assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + B * n:] == SENT).all())
    err = SU.err_of(x, want)
    print("inv_ctx %s: %.2e of scale (bar 1e-05)" % (case.id, err))
    assert err <= 1e-5
    _hip.call("cf_flow_step_inv_ctx", None, None, None, None, case.mode, 0, C, H, H, n, st)


@pytest.mark.gpu
@pytest.mark.parametrize("fxname", ["mnist_onehot", "mnist_embed_probsample_cf", "cifar10_eye", "cifar10_eye_vardeq_cf"])
def test_flow_step_inv_ctx_against_the_layer_path(L, fxname):
    """5b. Every specialist Coupling of an mnist and a cifar10 model, with and without contextflow (bias modes 1 and 2, the four
    geometries), on the trace's output of that layer: the one-launch inverse within 2e-5 of scale of the layer-by-layer
    Coupling.reverse(z, context) it replaces inside the differentiable walk.
    Measured on an MI355X: 2.7e-7, 2.2e-7, 2.6e-7, 3.1e-7 of scale."""
    from contextflow_amd.layers.autograd_inverse import _coupling_ctx_inverse
    p = SU.problem(fxname, 4)
    model = SU.build_specialist(p)
    mods = model.sequence_modules
    cd = p.context.to(DEV)
    seen, worst = set(), 0.0
    with torch.no_grad(), model._pinned(SU.fixture_noise(p), cd):
        for i, op in enumerate(p.ops):
            if op[0] != "coupling":
                continue
            m = mods[op[1]]
            z = p.inputs[i + 1].float().to(DEV)
            assert type(m) is L.Coupling and m.context_net and m._fused_ctx_ok(z)
            one, rec = _coupling_ctx_inverse(m, z, cd)
            layers = m.reverse(z, cd)
            assert rec.kind == "inv_coupling_ctx" and rec.mode == (1 if p.ctx["contextflow"] else 2)
            seen.add(tuple(z.shape[1:]))
            e = SU.err_of(one, layers)
            worst = max(worst, e)
            assert e <= 2e-5, (op[1], e)
    print("%s: %d geometries, fused against layer-by-layer: %.2e of scale (bar 2e-05)" % (fxname, len(seen), worst))
    assert seen == ({(8, 16, 16), (32, 8, 8)} if p.name == "mnist" else {(16, 16, 16), (32, 8, 8), (64, 4, 4)})


@pytest.mark.gpu
@pytest.mark.parametrize("case", U.BWD_CASES, ids=ids(U.BWD_CASES))
def test_flow_step_inv_bwd_ctx_data_per_geometry(L, case):
    """6. cf_flow_step_inv_bwd_ctx_data at the exact coupling input x (dense, and a channel slice of a wider tensor) under the drawn
    gx, against fp64 autograd through coupling_inv_ref with the bias: bar = step_fp64_ref.bar(error of fp32 CPU autograd on the same
    graph) = min(1e-4, max(2e-6, 4 x floor)) of the largest entry; sentinels framing gz intact; two launches the same bits.
    Measured on an MI355X: 1.2e-7 .. 6.1e-7 against floors of 5.1e-8 .. 3.2e-7 (bar 2.0e-6 in every case)."""
    from contextflow_amd.layers import _hip
    P, st = _hip.p, _hip.stream()
    d, ref = U.drawn(case)
    B, C, H = case.B, case.C, case.H
    HW = H * H
    gx = d["gz"]
    want = U.coupling_inv_ref(d, ref["z"], case.mode, gx=gx)["gz"]
    floor = U.coupling_inv_floor(d, ref["z"], case.mode, gx, want)
    ws, wsb = _coupling_tables(case, d["p"], bwd=True)
    x = d["big"].to(DEV)[:, :C] if d["big"] is not None else d["x"].to(DEV)
    xv, xbs = _hip.bview(x)
    assert xv.data_ptr() == x.data_ptr() and xbs == (2 if case.sliced and B > 1 else 1) * C * HW
    gxd, sb = gx.to(DEV), d["sbias"].to(DEV)
    PAD, SENT = 64, 12345.0
    outs = []
    for _ in range(2):
        buf = torch.full((B * C * HW + 2 * PAD,), SENT, device=DEV)
        gz = buf[PAD: PAD + B * C * HW].view(B, C, H, H)
        _hip.call("cf_flow_step_inv_bwd_ctx_data", P(xv), P(gxd), P(ws), P(wsb), P(sb), case.mode, P(gz), B, C, H, H, xbs, st)
        torch.cuda.synchronize()
        assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + B * C * HW:] == SENT).all())
        outs.append(gz)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    err, b = R.rel_err(outs[0], want), R.bar(floor)
    print("inv_bwd_ctx %s: err %.3e floor %.3e bar %.3e" % (case.id, err, floor, b))
    assert err <= b, "%s: err %.3e > bar %.3e (floor %.3e)" % (case.id, err, b, floor)
    _hip.call("cf_flow_step_inv_bwd_ctx_data", None, None, None, None, None, case.mode, None, 0, C, H, H, C * HW, st)


def _inv_bwd_call(gx, m1, Wm, m2, logs, out, B, C, H, W, unsq):
    from contextflow_amd.layers import _hip
    P = _hip.p
    _hip.call("cf_affine_ctx_inv_bwd_data", P(gx), P(m1), P(Wm), P(m2), P(logs), P(out), B, C, H, W, unsq, _hip.stream())


@pytest.mark.gpu
@pytest.mark.parametrize("C,H,W", SHAPES)
def test_affine_ctx_inv_bwd_data_against_fp64(L, C, H, W):
    """7. cf_affine_ctx_inv_bwd_data: gz = exp(l_b) (W_b^-T gx) against the fp64 formula (torch.linalg.solve on W_b^T) on the shapes
    and operands of test_affine_ctx_inv_against_fp64 - the three image levels, mnist's level, SMAP's 26 and ATM's 76 channels (the
    last above 64 KiB of LDS); B in {1, 5, 9}; with and without Wm / logs; m1 = NULL; m2 = NULL; gx_unsqueezed where C % 4 == 0
    (bitwise the plain call on squeeze_op(gx)); a gx 4 bytes off 16-byte alignment; sentinels behind gz; B = 0.  m1 = 0.1 randn:
    bar 2e-5 max(1, max|ref|).  One harder pass with m1 = 0.3 randn: max(2e-5, 3 x the fp32 solve's error the test computes).
    Measured on an MI355X: at most 0.008 of the bar on the 0.1 operands at every shape; the harder pass under contextflow 5.1e-7,
    5.2e-7, 2.3e-6, 1.1e-7, 2.4e-7, 1.0e-6, 2.0e-7 of scale over the seven shapes against fp32 solves of 4.4e-7, 2.2e-6, 2.3e-6,
    1.8e-7, 6.6e-7, 3.3e-5, 6.1e-6."""
    from contextflow_amd.layers import _hip
    from contextflow_amd.layers.squeeze import squeeze_op
    g = torch.Generator().manual_seed(C * 131 + H)
    n, PAD, worst = C * H * W, 64, 0.0
    d = lambda v: None if v is None else v.to(DEV).contiguous()
    for B in (1, 5, 9):
        gx, m1, m2, Wm, logs, _, _ = _operands(C, H, W, B, g, 0.1)
        flat = torch.zeros(B * n + 4, device=DEV)
        flat[1:1 + B * n] = gx.reshape(-1).to(DEV)
        layouts = {"dense": gx.to(DEV), "misaligned": flat[1:1 + B * n].view(B, C, H, W)}
        assert layouts["misaligned"].data_ptr() % 16 == 4
        for cf in (True, False):
            for half in ("both", "conv", "act"):
                a1, aW = (m1, Wm if cf else None) if half != "act" else (None, None)
                a2, al = (m2, logs if cf else None) if half != "conv" else (None, None)
                ref = U.affine_inv_bwd_ref(gx, a1, aW, a2, al)
                bar = 2e-5 * max(1.0, ref.abs().max().item())
                plain = None
                for lay, gv in layouts.items():
                    for unsq in ((0, 1) if C % 4 == 0 else (0,)):
                        if lay != "dense" and (unsq or half != "both"):
                            continue
                        buf = torch.full((B * n + PAD,), -77.0, device=DEV)
                        # gx_unsqueezed: the same numbers in the layout in front of the Squeeze((2,2))
                        src = squeeze_op(gv, (2, 2), True).contiguous() if unsq else gv
                        _inv_bwd_call(src, d(a1), d(aW), d(a2), d(al), buf, B, C, H, W, unsq)
                        assert torch.equal(buf[B * n:], torch.full((PAD,), -77.0, device=DEV)), (B, cf, half, lay, unsq)
                        out = buf[:B * n].view(B, C, H, W)
                        if unsq:
                            assert torch.equal(out, plain), (B, cf, half)
                            continue
                        if lay == "dense":
                            plain = out
                        err = (out.cpu().double() - ref).abs().max().item()
                        worst = max(worst, err / bar)
                        assert err <= bar, (B, cf, half, lay, err, bar)
    print("cf_affine_ctx_inv_bwd_data (%d,%d,%d): worst error / bar %.3f" % (C, H, W, worst))
    B = 5
    gx, m1, m2, Wm, logs, _, _ = _operands(C, H, W, B, g, 0.3)
    for cf in (True, False):
        aW, al = (Wm, logs) if cf else (None, None)
        ref = U.affine_inv_bwd_ref(gx, m1, aW, m2, al)
        sc = max(1.0, ref.abs().max().item())
        floor = (U.affine_inv_bwd_ref(gx, m1, aW, m2, al, torch.float32).double() - ref).abs().max().item() / sc
        bar = max(2e-5, 3.0 * floor)
        out = torch.empty(B, C, H, W, device=DEV)
        _inv_bwd_call(gx.to(DEV), d(m1), d(aW), d(m2), d(al), out, B, C, H, W, 0)
        err = (out.cpu().double() - ref).abs().max().item() / sc
        print("cf_affine_ctx_inv_bwd_data (%d,%d,%d) m1 = 0.3 randn, contextflow %d: %.2e of scale, fp32 floor %.2e, bar %.2e"
              % (C, H, W, cf, err, floor, bar))
        assert err <= bar, (cf, err, floor, bar)
    N = _hip.p(None)
    assert _hip.lib().cf_affine_ctx_inv_bwd_data(N, N, N, N, N, N, 0, C, H, W, 0, N) == 0


def _recording(monkeypatch):
    from contextflow_amd.layers import _hip
    names, real = [], _hip.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_hip, "call", recording)
    return names


def _latents(p, grad=True):
    return [t.float().to(DEV).requires_grad_(grad) for t in list(p.halves) + [p.z]]


@pytest.mark.gpu
@pytest.mark.parametrize("fxname", U.GRAD_FIXTURES)
def test_whole_walk_against_fp64_autograd(L, fxname, monkeypatch):
    """8. decode(trace latents, context, noise=fixture noise, differentiable=True) + backward under the fixed random gx against fp64
    autograd through the restated chain.  Per latent: max|got - ref| / max|ref| below max(1e-4, 3 x the fp32 CPU floor of the same
    graph).  Forward value against the fp64 restatement: max(1e-5, 3 x the fp32 restatement's error) of max(1, max|x|).  One
    cf_flow_step_inv_ctx / cf_flow_step_inv_bwd_ctx_data per coupling, one cf_affine_ctx_inv / cf_affine_ctx_inv_bwd_data per pair,
    no layer-by-layer conditioner and no parameter gradient.
    Measured on an MI355X, worst latent (its fp32 floor) and forward value: mnist_onehot 1.8e-6 (1.3e-6) / 8.9e-7, cifar10_eye 1.8e-6
    (8.6e-7) / 1.3e-6, cifar10_eye_vardeq_cf 1.0e-6 (4.8e-6) / 1.1e-6, cifar10_embed_eyesample 8.2e-7 (4.0e-7) / 7.0e-7,
    mnist_embed_probsample_cf 6.5e-7 (1.9e-6) / 1.5e-6, cifar10_eye_argmax_cf 1.3e-6 (4.0e-6) / 2.0e-6."""
    p = SU.problem(fxname, 4)
    gx, x64, ref, floor, fwd_floor = U.chain_reference(fxname)
    model = SU.build_specialist(p)
    lat = _latents(p)
    names = _recording(monkeypatch)
    x = model.decode(lat, p.context.to(DEV), noise=SU.fixture_noise(p), differentiable=True)
    assert x.grad_fn is not None and tuple(x.shape) == tuple(x64.shape)
    (x * gx.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    fwd, fbar = SU.err_of(x, x64), max(1e-5, 3.0 * fwd_floor)
    print("specialist decode_grad %s forward: %.2e of scale %.1f (fp32 restatement %.2e, bar %.2e)"
          % (fxname, fwd, SU.scale_of(x64), fwd_floor, fbar))
    ncpl, npair = sum(o[0] == "coupling" for o in p.ops), len(SU.ctx_pairs(p.ops))
    assert names.count("cf_flow_step_inv_ctx") == ncpl == names.count("cf_flow_step_inv_bwd_ctx_data")
    assert names.count("cf_affine_ctx_inv") == npair == names.count("cf_affine_ctx_inv_bwd_data")
    assert names.count("cf_postprocess_inv_bwd") == 1
    # (cf_add_sample_bias: the layer-by-layer conditioner of a specialist coupling; the encoders' own flows launch none)
    assert not [n for n in names if n == "cf_add_sample_bias" or n.startswith("cf_wgrad") or "param_grads" in n], names
    assert all(q.grad is None for q in model.parameters())
    failed = [] if fwd <= fbar else [("forward", fwd, fbar)]
    order = ref[1:] + ref[:1], floor[1:] + floor[:1]
    for what, t, r, fl in zip(["half%d" % i for i in range(len(p.halves))] + ["z"], lat, *order):
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.is_contiguous()
        err = (t.grad.cpu().double() - r).abs().max().item() / r.abs().max().item()
        bar = max(1e-4, 3.0 * fl)
        print("specialist decode_grad %s %s: relative error %.3e, fp32 floor %.3e, bar %.3e" % (fxname, what, err, fl, bar))
        if not err < bar:
            failed.append((what, err, bar))
    assert not failed, failed


@pytest.mark.gpu
@pytest.mark.parametrize("fxname", SU.CHAIN_FIXTURES)
def test_pixels_of_the_differentiable_walk(L, fxname):
    """9. Dequantisation noise 0.5: floor() of the differentiable walk's output is the fixture's pixels, every one, on all seven chain
    fixtures (the fp32 CPU restatement flips none there: test_specialist_inverse.py::test_fp32_floor_of_the_chain_and_the_pixels);
    the forward value within max(1e-5, 3 x that restatement's error) of the trace's continuous input."""
    p = SU.problem(fxname, 4, True)
    model = SU.build_specialist(p)
    x = model.decode(_latents(p), p.context.to(DEV), noise=SU.fixture_noise(p), differentiable=True)
    assert x.grad_fn is not None
    wrong = int((x.detach().floor().cpu() != p.x).sum())
    e = SU.err_of(x, p.inputs[1])
    print("%s: %d of %d pixels wrong, continuous point %.2e of scale" % (fxname, wrong, p.x.numel(), e))
    assert wrong == 0


@pytest.mark.gpu
def test_plumbing_of_the_flag(L):
    """10a. cifar10_eye_vardeq_cf (a stochastic encoder in every context layer): grad_fn only with a latent that requires a gradient;
    under no_grad the same values without one; gradients reach z and every half, no parameter gets a .grad; a second backward
    raises; the same noise= twice gives equal bits in x and in the gradients, fresh codes do not; an empty batch."""
    p = SU.problem("cifar10_eye_vardeq_cf", 4)
    model = SU.build_specialist(p)
    cd, n = p.context.to(DEV), SU.fixture_noise(p)
    assert model._stochastic_encoders()
    gx = torch.randn(p.x.shape, generator=torch.Generator().manual_seed(2)).to(DEV)

    def run():
        lat = _latents(p)
        x = model.decode(lat, cd, noise=n, differentiable=True)
        (x * gx).sum().backward()
        return x, lat
    x, lat = run()
    assert x.grad_fn is not None and all(t.grad is not None and t.grad.shape == t.shape and bool(t.grad.abs().max() > 0) for t in lat)
    assert all(q.grad is None for q in model.parameters())
    assert all(e.fixed_noise is None for e in model._stochastic_encoders())
    with pytest.raises(RuntimeError):
        (x * gx).sum().backward()
    x2, lat2 = run()
    assert torch.equal(x, x2) and all(torch.equal(a.grad, b.grad) for a, b in zip(lat, lat2))
    plain = model.decode(_latents(p, False), cd, noise=n, differentiable=True)
    with torch.no_grad():
        quiet = model.decode(_latents(p), cd, noise=n, differentiable=True)
    assert plain.grad_fn is None and quiet.grad_fn is None and torch.equal(plain, x.detach()) and torch.equal(quiet, plain)
    assert not torch.equal(model.decode(_latents(p, False), cd, differentiable=True), plain)          # fresh codes without noise=
    # only z requires a gradient: the halves get none
    lat3 = _latents(p, False)
    lat3[-1].requires_grad_(True)
    x3 = model.decode(lat3, cd, noise=n, differentiable=True)
    (x3 * gx).sum().backward()
    assert torch.equal(lat3[-1].grad, lat[-1].grad) and all(t.grad is None for t in lat3[:-1])
    # an empty batch
    e = [t[:0].detach().clone().requires_grad_(True) for t in lat]
    xe = model.decode(e, cd[:0], noise=[t[:0] for t in n], differentiable=True)
    assert tuple(xe.shape) == (0,) + tuple(p.x.shape[1:])
    xe.sum().backward()
    assert all(t.grad is not None and t.grad.shape == t.shape for t in e)


@pytest.mark.gpu
def test_inverse_on_mnist(L):
    """10b. inverse(z, context, noise=, differentiable=True) on mnist_onehot (no SplitPrior): the values of decode([z]) bit for bit,
    and the z gradient of the whole-walk test's reference within its bar."""
    fxname = "mnist_onehot"
    p = SU.problem(fxname, 4)
    gx, x64, ref, floor, _ = U.chain_reference(fxname)
    assert not p.halves
    model = SU.build_specialist(p)
    cd, n = p.context.to(DEV), SU.fixture_noise(p)
    z = p.z.float().to(DEV).requires_grad_(True)
    x = model.inverse(z, cd, noise=n, differentiable=True)
    assert x.grad_fn is not None
    assert torch.equal(x.detach(), model.decode([z.detach()], cd, noise=n, differentiable=True))
    (x * gx.float().to(DEV)).sum().backward()
    err = (z.grad.cpu().double() - ref[0]).abs().max().item() / ref[0].abs().max().item()
    print("specialist inverse mnist_onehot z: relative error %.3e, fp32 floor %.3e" % (err, floor[0]))
    assert err < max(1e-4, 3.0 * floor[0])


@pytest.mark.gpu
def test_refusals(L):
    """10c. What keeps raising: a context for a flow without context nets; return_logp on a specialist flow in either form;
    clamp=True; a specialist flow without its context, also on the differentiable path; a context layer without a rule -
    TransCoupling(c) (a smap specialist) and a Coupling(c) outside the fused geometry (smap with the time-series conv coupling) -
    by name and index."""
    import contextflow_amd as cfa
    from tests.gpu_util import build_model
    from tests.sample_logp_util import problem
    _, params, z, _, _, _, _, _ = problem("mnist")
    gen = build_model("mnist", params)
    zg = z.float().to(DEV).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="context"):
        gen.inverse(zg, context=torch.zeros(zg.shape[0], 1, device=DEV), differentiable=True)
    p = SU.problem("mnist_onehot", 4)
    model = SU.build_specialist(p)
    cd, n, lat = p.context.to(DEV), SU.fixture_noise(p), _latents(p)
    with pytest.raises(NotImplementedError):
        model.decode(lat, cd, noise=n, return_logp=True)
    with pytest.raises(NotImplementedError):
        model.inverse(lat[-1], cd, noise=n, return_logp=True)
    with pytest.raises(NotImplementedError, match="return_logp"):
        model.decode(lat, cd, noise=n, return_logp=True, differentiable=True)
    with pytest.raises(NotImplementedError, match="return_logp"):
        model.inverse(lat[-1], cd, noise=n, return_logp=True, differentiable=True)
    with pytest.raises(ValueError, match="clamp"):
        model.decode(lat, cd, noise=n, clamp=True, differentiable=True)
    with pytest.raises(ValueError, match="context"):
        model.decode(lat, differentiable=True)
    with pytest.raises(ValueError, match="context"):
        model.inverse(lat[-1], differentiable=True)
    for coupling, word in (("trans", "TransCoupling"), ("conv", "Coupling")):
        cfg, ds, MM = cfa.preset_config("smap", coupling=coupling)
        cfg.update(generalist=False, contextflow=True)
        torch.manual_seed(1)
        flow = cfa.create_model(cfg, ds, MM, contexts=[3]).to(DEV).eval()
        last = len(flow.sequence_modules) - 1
        assert type(flow.sequence_modules[last]).__name__ == word
        zz = torch.randn(2, *flow.dist.mG.shape[2:], generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_(True)
        with pytest.raises(NotImplementedError, match=r"%s with a context net \(layer %d\)" % (word, last)):
            flow.decode([zz], torch.zeros(2, 1, dtype=torch.long, device=DEV), differentiable=True)
