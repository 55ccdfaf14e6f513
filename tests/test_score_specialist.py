"""The input gradient of log p(x | c): `FlowSequential.score(x, context=...)` and a differentiable `log_prob` for the specialist
(context-conditioned) flows, and the three data-only kernels under them.

GPU tests go through the C ABI like tests/test_gpu_parity.py; the reference is torch.autograd through the fp64 CPU oracle on the
fixtures' own samples, noise, contexts and parameters (4 samples, or 9 rows built from them: a ragged last group in every
kernel that groups samples)."""
import types

import pytest
import torch

from oracle import flow_oracle as fo
from tests.helpers import bpd, load_specialist

pytestmark = pytest.mark.gpu

BPD_TOL = 1e-5
DEV = "cuda:0"
IDX9 = [0, 1, 2, 3, 0, 1, 2, 3, 1]
FIXTURES = ["mnist_eye_cf", "cifar10_onehot_cf", "smap_onehot_cf", "atm_onehot_cf", "mnist_onehot", "cifar10_eye",
            "cifar10_embed_eyesample", "cifar10_eye_vardeq_cf", "smap_eye", "mnist_embed_probsample_cf", "cifar10_eye_argmax_cf"]


@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


_CASES = {}


def _case(fxname, B):
    """Inputs and the oracle's answers of one (fixture, batch), computed once: ref = d sum(w logp) / dx by fp64 autograd, floor =
    the relative error fp32 autograd makes through the same oracle, lp = the fp64 log-densities."""
    if (fxname, B) in _CASES:
        return _CASES[fxname, B]
    name, ctx, ops, M, params, inp = load_specialist(fxname)
    idx = torch.tensor({4: [0, 1, 2, 3], 9: IDX9}[B])
    rows = lambda t: t[idx] if t.shape[0] == inp["x"].shape[0] else t       # (the time-series fixtures carry a placeholder u)
    x, u, context = rows(inp["x"]), rows(inp["u"]), rows(inp["context"])
    eps, cnoise = [rows(e) for e in inp["eps"]], [rows(c) for c in inp["cnoise"]]
    wts = torch.randn(B, M, generator=torch.Generator().manual_seed(33))
    p64 = {k: (v.double() if v.is_floating_point() else v) for k, v in params.items()}
    x64 = x.double().requires_grad_(True)
    _, lp = fo.flow_forward(ops, p64, x64, u.double(), [e.double() for e in eps], ctx=ctx, context=context,
                            cnoise=[c.double() for c in cnoise])
    (lp * wts.double()).sum().backward()
    ref = x64.grad
    x32 = x.clone().requires_grad_(True)
    _, lp32 = fo.flow_forward(ops, params, x32, u, eps, ctx=ctx, context=context, cnoise=cnoise)
    (lp32 * wts).sum().backward()
    scale = ref.abs().max().item()
    floor = (x32.grad.double() - ref).abs().max().item() / scale
    assert torch.isfinite(ref).all() and scale > 0.0
    c = types.SimpleNamespace(fxname=fxname, name=name, ctx=ctx, M=M, params=params, x=x, u=u, eps=eps, context=context, cnoise=cnoise,
                              wts=wts, ref=ref, scale=scale, floor=floor, tol=max(1e-4, 3.0 * floor), lp=lp.detach())
    _CASES[fxname, B] = c
    return c


def _model(c, train=False, frozen=True):
    import contextflow_amd as cfa
    from tests.gpu_util import set_noise
    cfg, ds, MM = cfa.preset_config(c.name)
    enc_type = c.ctx.get("enc_type", "uniform")
    cfg.update(generalist=False, enc_emb=c.ctx["enc_emb"], enc_type=enc_type, contextflow=c.ctx["contextflow"])
    model = cfa.create_model(cfg, ds, MM, contexts=c.ctx["contexts"])
    model.load_state_dict({k: v.clone() for k, v in c.params.items()}, strict=True)
    model = model.to(DEV)
    model = model.train() if train else model.eval()
    if frozen:
        for p in model.parameters():
            p.requires_grad_(False)
    set_noise(model, c.u, c.eps)
    noisy = cfa.layers.UniformCatDequantization if enc_type == "uniform" else cfa.layers.ConditionalGaussianDistribution
    encs = [m for m in model.modules() if isinstance(m, noisy)]
    assert len(encs) == len(c.cnoise)
    for e, n in zip(encs, c.cnoise):
        e.fixed_noise = n.to(DEV)
    return model


def _check_against_oracle(c, tag):
    model = _model(c)
    xd, cd, wd = c.x.to(DEV).requires_grad_(True), c.context.to(DEV), c.wts.to(DEV)
    z, logp = model(xd, cd)
    assert logp.requires_grad and not z.requires_grad
    (logp * wd).sum().backward()
    assert xd.grad is not None and xd.grad.shape == xd.shape and xd.grad.dtype == torch.float32
    grad, logp2 = model.score(c.x.to(DEV), weights=wd, context=cd)
    assert torch.equal(grad, xd.grad) and torch.equal(logp2, logp.detach())
    assert all(p.grad is None for p in model.parameters())
    btol = max(BPD_TOL, 1e-5 * bpd(c.lp.float(), c.name).abs().max().item())
    berr = (bpd(logp.detach().cpu(), c.name) - bpd(c.lp.float(), c.name)).abs().max().item()
    err = (grad.cpu().double() - c.ref).abs().max().item() / c.scale
    print("specialist score %s %s B=%d: relative error %.3e, fp32 floor %.3e, bar %.3e; bits/dim error %.3e (bar %.1e)"
          % (tag, c.fxname, c.x.shape[0], err, c.floor, c.tol, berr, btol))
    assert berr < btol
    assert torch.isfinite(grad).all()
    assert err < c.tol, "relative input-gradient error %.3e (fp32 floor %.3e, bar %.1e)" % (err, c.floor, c.tol)


# ------------------------------------------------------------------------------------------ 1. against the fp64 oracle
@pytest.mark.parametrize("fxname", FIXTURES)
def test_specialist_input_gradient_against_autograd_oracle(L, fxname):
    """d sum(w * logp) / dx of a frozen specialist - x.requires_grad through `forward` + backward, and `score(x, weights=w,
    context=c)`, bitwise equal - against torch.autograd through the fp64 oracle on the fixture's 4 samples with its noise and
    contexts.  Error = max|got - ref| / max|ref|; bar = max(1e-4, 3 x the error fp32 torch.autograd makes through the same
    oracle); bits/dim of logp within the bar of test_specialist_backward_against_autograd_oracle; no parameter gradient.
    Measured on an MI355X, error (fp32 floor of that machine's CPU): mnist_eye_cf 1.8e-5 (2.0e-5), cifar10_onehot_cf 1.30e-4
    (1.54e-4), smap_onehot_cf 2.0e-6 (1.3e-5), atm_onehot_cf 2.4e-6 (3.5e-5), mnist_onehot 2.0e-5 (2.0e-5), cifar10_eye 9.1e-5
    (1.08e-4), cifar10_embed_eyesample 2.42e-4 (1.97e-4), cifar10_eye_vardeq_cf 9.3e-5 (1.61e-4), smap_eye 1.2e-6 (1.2e-6),
    mnist_embed_probsample_cf 1.7e-5 (3.8e-5), cifar10_eye_argmax_cf 1.77e-4 (1.30e-4)."""
    _check_against_oracle(_case(fxname, 4), "B4")


# ------------------------------------------------------------------------------------------ 2. ragged batches
@pytest.mark.parametrize("fxname", ["cifar10_onehot_cf", "cifar10_eye", "mnist_eye_cf"])
def test_specialist_input_gradient_ragged_batches(L, fxname):
    """The same at B = 9 (rows 0,1,2,3,0,1,2,3,1 of the fixture): a ragged last group in the wave affine kernel (4 samples per
    workgroup), the mixture kernel (S = 4), the 8x8 step tile (2) and the 4x4 step tile (8).  cifar10_onehot_cf: mode 1, wave
    affine shapes, table mixtures; cifar10_eye: mode 2; mnist_eye_cf: the LDS affine form.
    Measured: cifar10_onehot_cf 5.9e-5 (7.6e-5), cifar10_eye 8.6e-5 (7.6e-5), mnist_eye_cf 9.6e-5 (9.6e-5)."""
    _check_against_oracle(_case(fxname, 9), "B9")


# ------------------------------------------------------------------------------------------ 3. training walk + x.requires_grad
@pytest.mark.parametrize("fxname", ["cifar10_onehot_cf", "cifar10_eye"])
def test_training_walk_returns_the_input_gradient_too(L, fxname):
    """train(), parameters trainable: the training walk goes on through the pre-processing when x requires a gradient - the
    parameter gradients are bitwise those of the call without it, x.grad is within the bar of test 1."""
    c = _case(fxname, 4)
    model = _model(c, train=True, frozen=False)
    cd, wd = c.context.to(DEV), c.wts.to(DEV)

    def run(xgrad):
        model.zero_grad(set_to_none=True)
        xd = c.x.to(DEV).requires_grad_(xgrad)
        _, logp = model(xd, cd)
        assert logp.requires_grad
        (logp * wd).sum().backward()
        torch.cuda.synchronize()
        return xd.grad, logp.detach(), {k: (p.grad.clone() if p.grad is not None else None) for k, p in model.named_parameters()}

    gx, lp_a, gp_a = run(True)
    none, lp_b, gp_b = run(False)
    assert none is None and gx is not None and torch.equal(lp_a, lp_b)
    assert sum(v is not None for v in gp_a.values()) >= 20
    for k, v in gp_a.items():
        assert (v is None) == (gp_b[k] is None), k
        if v is not None:
            assert torch.equal(v, gp_b[k]), k
    err = (gx.cpu().double() - c.ref).abs().max().item() / c.scale
    print("specialist training walk %s: x.grad relative error %.3e, fp32 floor %.3e, bar %.3e" % (fxname, err, c.floor, c.tol))
    assert err < c.tol


# ------------------------------------------------------------------------------------------ 4. the affine kernel alone
def _affine_ref(gz, m1, Wm, m2, logs):
    B, C = gz.shape[:2]
    g = gz.double().reshape(B, C, -1)
    if m2 is not None:
        lb = m2[:, C:].double() + (logs.double() if logs is not None else 0.0)
        g = g * torch.exp(-lb)[:, :, None]
    if m1 is not None:
        M1 = m1.double().view(B, C, C)
        Wb = torch.tril(M1, -1) + torch.diag_embed(torch.exp(torch.diagonal(M1, dim1=1, dim2=2)))
        if Wm is not None:
            Wb = Wb + Wm.double() - torch.eye(C, dtype=torch.float64)
        g = torch.bmm(Wb.transpose(1, 2), g)
    return g.reshape(gz.shape)


@pytest.mark.parametrize("C,H,W", [(16, 16, 16), (32, 8, 8), (64, 4, 4), (8, 16, 16), (26, 8, 1), (76, 18, 1),
                                     (76, 12, 12)])                                       # > 64 KiB of LDS
def test_affine_ctx_bwd_data_against_fp64(L, C, H, W):
    """cf_affine_ctx_bwd_data: gx = W_b^T (gz exp(-l_b)) against the fp64 formula at the three wave shapes, mnist's level, SMAP's
    26 and ATM's 76 channels; B in {1, 5, 9}; with and without Wm / logs; m1 = NULL; m2 = NULL; out_unsqueeze where C % 4 == 0
    (bitwise squeeze_op(..., reverse) of the plain result); a batch-strided gz; a 4-byte-misaligned gz (the generic form);
    sentinels behind gx.  Bar: 2e-5 max(1, max|ref|), as the forward twin's."""
    from contextflow_amd.layers import _hip
    from contextflow_amd.layers.squeeze import squeeze_op
    P, st = _hip.p, _hip.stream()
    g = torch.Generator().manual_seed(C * 131 + H)
    r = lambda *sh: torch.randn(*sh, generator=g)
    n, PAD, worst = C * H * W, 64, 0.0
    for B in (1, 5, 9):
        gz, m1, m2 = r(B, C, H, W), 0.3 * r(B, C * C), 0.3 * r(B, 2 * C)
        Wm, logs = torch.linalg.qr(r(C, C))[0].contiguous(), 0.2 * r(C)
        wide = torch.cat([gz, r(B, C, H, W)], 1).to(DEV)                     # gz as a channel slice: batch stride 2 C H W
        flat = torch.zeros(B * n + 4, device=DEV)
        flat[1:1 + B * n] = gz.reshape(-1).to(DEV)
        layouts = {"dense": (gz.to(DEV), n), "strided": (wide[:, :C], 2 * n), "misaligned": (flat[1:1 + B * n].view(B, C, H, W), n)}
        assert layouts["misaligned"][0].data_ptr() % 16 == 4
        d = lambda v: None if v is None else v.to(DEV).contiguous()
        for cf in (True, False):
            for half in ("both", "conv", "act"):
                a1, aW = (m1, Wm if cf else None) if half != "act" else (None, None)
                a2, al = (m2, logs if cf else None) if half != "conv" else (None, None)
                ref = _affine_ref(gz, a1, aW, a2, al)
                bar = 2e-5 * max(1.0, ref.abs().max().item())
                plain = None
                for lay, (gv, gbs) in layouts.items():
                    for unsq in ((0, 1) if C % 4 == 0 else (0,)):
                        if lay != "dense" and (unsq or half != "both"):
                            continue
                        buf = torch.full((B * n + PAD,), -77.0, device=DEV)
                        _hip.call("cf_affine_ctx_bwd_data", P(gv), P(d(a1)), P(d(aW)), P(d(a2)), P(d(al)), P(buf), B, C, H, W, gbs,
                                  unsq, st)
                        assert torch.equal(buf[B * n:], torch.full((PAD,), -77.0, device=DEV)), (B, cf, half, lay, unsq)
                        out = buf[:B * n]
                        if unsq:
                            assert torch.equal(squeeze_op(plain, (2, 2), True), out.view(B, C // 4, 2 * H, 2 * W)), (B, cf, half)
                            continue
                        out = out.view(B, C, H, W)
                        if lay == "dense":
                            plain = out
                        err = (out.cpu().double() - ref).abs().max().item()
                        worst = max(worst, err / bar)
                        assert err <= bar, (B, cf, half, lay, err, bar)
    print("cf_affine_ctx_bwd_data (%d,%d,%d): worst error / bar %.3f" % (C, H, W, worst))
    N = _hip.p(None)
    assert _hip.lib().cf_affine_ctx_bwd_data(N, N, N, N, N, N, 0, C, H, W, n, 0, N) == 0


# ------------------------------------------------------------------------------------------ 5. bitwise twins
@pytest.mark.parametrize("D,H,W", [(3, 1, 1), (8, 4, 4), (4, 7, 7)])
def test_gmm_ctx_bwd_data_is_bitwise_the_training_form(L, D, H, W):
    """cf_gmm_ctx_bwd_data against cf_gmm_ctx_bwd / cf_gmm_ctx_bwd_tab: both forms, with and without the kept log-joints, h w in
    {1, 16, 49}, B in {1, 5} (one ragged group of S = 4): the same gx, bit for bit."""
    from contextflow_amd.layers import _hip
    P, st = _hip.p, _hip.stream()
    g = torch.Generator().manual_seed(D * 100 + H)
    M, K, U, HW = 3, 2, 3, H * W
    MK = M * K
    d = lambda t: t.contiguous().to(DEV)
    mG, sG = d(0.5 * torch.randn(M, K, D, H, W, generator=g)), d(0.5 * torch.randn(M, K, D, H, W, generator=g) + 0.5)
    logw = d(torch.log_softmax(torch.randn(M, K, generator=g), -1))
    cs_tab = 0.3 * torch.randn(U, MK, D, generator=g)
    inv, dsg = torch.empty(U, MK * D * HW, device=DEV), torch.empty(U, MK * D * HW, device=DEV)
    lsum = torch.empty(U, MK, device=DEV)
    _hip.call("cf_gmm_ctx_tables", P(sG), P(d(cs_tab)), P(inv), P(dsg), P(lsum), U, MK, D, HW, st)
    for B in (1, 5):
        x, gout = d(torch.randn(B, D, H, W, generator=g)), d(torch.randn(B, M, generator=g))
        key = torch.randint(0, U, (B,), generator=g)
        c = 0.3 * torch.randn(B, 2, M, K, D, generator=g)
        c[:, 1] = cs_tab[key].reshape(B, M, K, D)
        c, key = d(c), key.to(torch.int32).to(DEV)
        out, lp = torch.empty(B, M, device=DEV), torch.empty(B, MK, device=DEV)
        _hip.call("cf_gmm_ctx_logprob", P(x), P(mG), P(sG), P(logw), P(c), P(out), P(lp), B, M, K, D, HW, D * HW, 0, st)
        for kept in (lp, None):
            for tab in (False, True):
                gx = torch.full((B, D, H, W), float("nan"), device=DEV)
                gc = torch.empty(B, 2 * MK * D, device=DEV)
                gd = torch.full((B * D * HW + 32,), -77.0, device=DEV)
                if tab:
                    _hip.call("cf_gmm_ctx_bwd_tab", P(x), P(mG), P(inv), P(dsg), P(lsum), P(logw), P(c), P(key), P(gout), P(kept), P(gx),
                              P(gc), B, M, K, D, HW, D * HW, st)
                    _hip.call("cf_gmm_ctx_bwd_data", P(x), P(mG), None, P(inv), P(lsum), P(logw), P(c), P(key), P(gout), P(kept), P(gd),
                              B, M, K, D, HW, D * HW, st)
                else:
                    _hip.call("cf_gmm_ctx_bwd", P(x), P(mG), P(sG), P(logw), P(c), P(gout), P(kept), P(gx), P(gc), B, M, K, D, HW,
                              D * HW, st)
                    _hip.call("cf_gmm_ctx_bwd_data", P(x), P(mG), P(sG), None, None, P(logw), P(c), None, P(gout), P(kept), P(gd),
                              B, M, K, D, HW, D * HW, st)
                assert torch.isfinite(gx).all() and float(gx.abs().max()) > 0.0
                assert torch.equal(gd[:B * D * HW].view_as(gx), gx), (B, tab, kept is None)
                assert torch.equal(gd[B * D * HW:], torch.full((32,), -77.0, device=DEV))
    N = _hip.p(None)
    assert _hip.lib().cf_gmm_ctx_bwd_data(N, N, N, N, N, N, N, N, N, N, N, 0, M, K, D, HW, D * HW, N) == 0


@pytest.mark.parametrize("C,H,W", [(16, 16, 16), (32, 8, 8), (64, 4, 4), (8, 16, 16)])
def test_flow_step_bwd_ctx_data_is_bitwise_the_training_form(L, C, H, W):
    """cf_flow_step_bwd_ctx_data (k_flow_step_bwd<G, CTX, DATA>: no s_gh plane) against cf_flow_step_bwd_ctx at the three image
    levels and mnist's, B in {3, 9} (ragged 8x8 and 4x4 tiles): the same gx, bit for bit."""
    from contextflow_amd.layers import _hip, Coupling
    from contextflow_amd.layers.coupling import identity_front_step_tables
    P, st, f = _hip.p, _hip.stream(), _hip.f32
    torch.manual_seed(C + H)
    cpl = Coupling(C, kernel_size=(3, 3), padding=(1, 1)).to(DEV)
    with torch.no_grad():
        for conv in (cpl.NN[0], cpl.NN[2], cpl.NN[4]):
            conv.weight.normal_(0.0, 0.08)
            conv.bias.normal_(0.0, 0.05)
    c1, c2, c3 = cpl.NN[0], cpl.NN[2], cpl.NN[4]
    ws = identity_front_step_tables(cpl, f(c1.weight.detach()), C, H, W, DEV)
    wsb = torch.empty(_hip.lib().cf_flow_step_bwd_ws_bytes(C, H, W), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_bwd_prepare", P(torch.eye(C, device=DEV)), P(torch.zeros(C, device=DEV)), P(f(c1.weight.detach())),
              P(f(c2.weight.detach())), P(f(c3.weight.detach())), P(wsb), C, H, W, st)
    g = torch.Generator().manual_seed(C * 7 + W)
    for B in (3, 9):
        x, gz = torch.randn(B, C, H, W, generator=g).to(DEV), torch.randn(B, C, H, W, generator=g).to(DEV)
        gld, sb = torch.randn(B, generator=g).to(DEV), (0.3 * torch.randn(B, C, generator=g)).to(DEV)
        gx = torch.full((B, C, H, W), float("nan"), device=DEV)
        s_gh = torch.empty(B, C, H * W, device=DEV)
        _hip.call("cf_flow_step_bwd_ctx", P(x), P(gz), P(gld), P(ws), P(wsb), P(sb), P(gx), None, None, None, P(s_gh), None, None, None,
                  B, C, H, W, C * H * W, st)
        gd = torch.full((B * C * H * W + 32,), -77.0, device=DEV)
        _hip.call("cf_flow_step_bwd_ctx_data", P(x), P(gz), P(gld), P(ws), P(wsb), P(sb), P(gd), B, C, H, W, C * H * W, st)
        assert torch.isfinite(gx).all() and float(gx.abs().max()) > 0.0
        assert torch.equal(gd[:B * C * H * W].view_as(gx), gx), B
        assert torch.equal(gd[B * C * H * W:], torch.full((32,), -77.0, device=DEV))
    N = _hip.p(None)
    assert _hip.lib().cf_flow_step_bwd_ctx_data(N, N, N, N, N, N, N, 0, C, H, W, C * H * W, N) == 0


# ------------------------------------------------------------------------------------------ 6. no parameter work
def test_specialist_score_launches_no_parameter_work(L, monkeypatch):
    """The entry points `score` passes to _hip.call on cifar10_onehot_cf, parameters trainable: one cf_affine_ctx_bwd_data per
    Conv1x1, one cf_flow_step_bwd_ctx_data per Coupling, one cf_gmm_ctx_bwd_data per prior, one cf_preprocess_bwd - and none of
    the training backward's kernels, no channel sums, no weight gradient."""
    from contextflow_amd.layers import _hip, Conv1x1, Coupling, SplitPrior
    c = _case("cifar10_onehot_cf", 4)
    model = _model(c, train=True, frozen=False)
    flags = [p.requires_grad for p in model.parameters()]
    assert any(flags)
    names = []
    real = _hip.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_hip, "call", recording)
    model.score(c.x.to(DEV), context=c.context.to(DEV))
    torch.cuda.synchronize()
    monkeypatch.undo()
    count = lambda cls: sum(isinstance(m, cls) for m in model.sequence_modules)
    assert count(Conv1x1) > 0 and names.count("cf_affine_ctx_bwd_data") == count(Conv1x1)
    assert count(Coupling) > 0 and names.count("cf_flow_step_bwd_ctx_data") == count(Coupling)
    assert names.count("cf_gmm_ctx_bwd_data") == count(SplitPrior) + 1
    assert names.count("cf_preprocess_bwd") == 1
    banned = {"cf_conv1x1_ctx_bwd", "cf_actnorm_ctx_bwd", "cf_flow_step_bwd_ctx", "cf_gmm_ctx_bwd", "cf_gmm_ctx_bwd_tab",
              "cf_gmm_ctx_pgrad_tab", "cf_sample_channel_sums"}
    assert not [n for n in names if n in banned or "wgrad" in n], names
    assert [p.requires_grad for p in model.parameters()] == flags and all(p.grad is None for p in model.parameters())


# ------------------------------------------------------------------------------------------ 7. semantics
def test_specialist_score_semantics(L):
    c = _case("cifar10_onehot_cf", 4)
    model = _model(c, train=True, frozen=False)
    B, M = c.x.shape[0], c.M
    flags = [p.requires_grad for p in model.parameters()]
    xd, cd = c.x.to(DEV), c.context.to(DEV)
    eye = torch.eye(M, device=DEV)
    g3, lp3 = model.score(xd, labels=3, context=cd)
    gw, lpw = model.score(xd, weights=eye[3].expand(B, M).contiguous(), context=cd)
    assert torch.equal(g3, gw) and torch.equal(lp3, lpw)
    assert g3.shape == xd.shape and g3.dtype == torch.float32 and float(g3.abs().max()) > 0.0
    lab = torch.tensor([0, 9, 3, 1])
    gl, _ = model.score(xd, labels=lab, context=cd)
    gw, _ = model.score(xd, weights=eye[lab.to(DEV)], context=cd)
    assert torch.equal(gl, gw)
    assert torch.equal(gl[2], g3[2]) and not torch.equal(gl[0], g3[0])
    gm, lpm = model.score(xd, context=cd)                 # the marginal: w = softmax of the returned logp
    gw, _ = model.score(xd, weights=torch.softmax(lpm, dim=1), context=cd)
    assert torch.equal(gm, gw) and torch.equal(lpm, lp3)
    with torch.no_grad():
        gn, lpn = model.score(xd, context=cd)
    assert torch.equal(gn, gm) and torch.equal(lpn, lpm)
    assert not gm.requires_grad and not lpm.requires_grad and xd.grad is None and not xd.requires_grad
    xr = c.x.to(DEV).requires_grad_(True)                # an input that requires a gradient keeps its flag and gets no .grad
    gr, _ = model.score(xr, context=cd)
    assert torch.equal(gr, gm) and xr.grad is None and xr.requires_grad and not gr.requires_grad
    assert [p.requires_grad for p in model.parameters()] == flags and all(p.grad is None for p in model.parameters())
    with pytest.raises(ValueError):
        model.score(xd, labels=3, weights=eye[3].expand(B, M), context=cd)
    with pytest.raises(ValueError):
        model.score(xd, labels=M, context=cd)
    with pytest.raises(NotImplementedError):
        model.score(xd)                                   # a specialist flow without its context
    g0, lp0 = model.score(xd[:0], context=cd[:0])
    assert tuple(g0.shape) == (0,) + tuple(xd.shape[1:]) and g0.dtype == torch.float32 and tuple(lp0.shape) == (0, M)
