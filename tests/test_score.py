"""The input gradient of log p(x): differentiable `log_prob` (x.requires_grad) and `FlowSequential.score`.

GPU tests go through the C ABI like tests/test_gpu_parity.py; the reference is torch.autograd through the fp64 CPU oracle
on the same inputs, noise and parameters.  The closed form of the pre-processing backward is pinned on the CPU."""
import pytest
import torch

from oracle import flow_oracle as fo
from tests.helpers import load_e2e, e2e_inputs, bpd, load_specialist

BPD_TOL = 1e-5
DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


def _inputs(name, B, seed):
    C, H, W = fo.CONFIGS[name][0]
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, H, W, generator=g) if name in ("smap", "atm") else torch.randint(0, 256, (B, C, H, W), generator=g).float()
    u = torch.rand(B, C, H, W, generator=g)
    eps = [torch.randn(B, 1, H, W, generator=g)]
    return x, u, eps, g


def _frozen(model, frozen=True):
    for p in model.parameters():
        p.requires_grad_(not frozen)
        p.grad = None
    return model


# ------------------------------------------------------------------------------------------ 6. the closed form (CPU)
def test_preprocess_backward_closed_form():
    """v = ((x + u) / s1 + t1) / s2 + t2, y = logit(v), ld = sum(-log v - log(1 - v)):
    gx = (gy (2 + e^y + e^-y) + gld (e^y - e^-y)) / (s1 s2), from y alone - what cf_preprocess_bwd implements - against
    torch.autograd through the oracle's own layers (affine x 2, logit) in fp64."""
    g = torch.Generator().manual_seed(3)
    B, C, H, W = 4, 3, 6, 5
    t1, s1, t2, s2 = 0.0, 256.0, 0.0001, 1.0002000400080016          # model.py:97-100 (oracle.flow_oracle.program)
    x = (torch.randint(0, 256, (B, C, H, W), generator=g).double() + torch.rand(B, C, H, W, generator=g).double()).requires_grad_(True)
    gy = torch.randn(B, C, H, W, generator=g).double()
    gld = torch.randn(B, generator=g).double()
    v, _ = fo.affine_fwd(x, t1, s1)
    v, _ = fo.affine_fwd(v, t2, s2)
    y, ld = fo.logit_fwd(v)
    ((gy * y).sum() + (gld * ld).sum()).backward()
    ref = x.grad
    yd = y.detach()
    s12 = float(torch.tensor([s1], dtype=torch.float32)) * float(torch.tensor([s2], dtype=torch.float32))   # affine_fwd: fp32 constants
    ep, em = torch.exp(yd), torch.exp(-yd)
    got = (gy * (2.0 + ep + em) + gld.view(B, 1, 1, 1) * (ep - em)) / s12
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    assert err < 1e-12, err


# ------------------------------------------------------------------------------------------ 1. against the fp64 oracle
@pytest.mark.gpu
@pytest.mark.parametrize("name,B,tag", [("mnist", 6, None), ("cifar10", 5, None), ("smap", 7, None), ("atm", 3, None),
                                        ("mnist", 5, "stress"), ("cifar10", 4, "stress"), ("smap", 6, "stress")])
def test_input_gradient_against_autograd_oracle(L, name, B, tag):
    """d sum(w * logp) / d x of a frozen model - x.requires_grad through `forward` + backward, and `score(x, weights=w)`,
    bitwise equal - against torch.autograd through the fp64 oracle on the same inputs, noise and weights (the cases of
    test_backward_against_autograd_oracle).  Error = max|got - ref| / max|ref|; bar = max(1e-4, 3 x the error fp32
    torch.autograd makes through the same oracle on the same inputs).
    Measured on an MI355X, error (fp32 floor of that machine's CPU): mnist 1.02e-4 (8.7e-5), cifar10 1.0e-5 (2.5e-5), smap
    5.4e-7 (8.0e-6), atm 1.7e-5 (3.5e-5); stress: mnist 1.8e-5 (1.8e-5), cifar10 3.6e-5 (3.6e-5), smap 7.7e-6 (1.0e-5)."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e(name, tag)
    x, u, eps, g = _inputs(name, B, 21)
    if tag:                      # the fixture's own samples: the mixture components sit on THEIR latents (moderate |logp|)
        fxx, fxu, fxe = e2e_inputs(name, fx)
        x, eps = fxx[:B], [e[:B] for e in fxe]
        u = fxu[:B] if fxu is not None else u
    wts = torch.randn(B, M, generator=g)
    # oracle: fp64 autograd, and the fp32 floor of the same graph
    p64 = {k: (v.double() if v.is_floating_point() else v) for k, v in params.items()}
    x64 = x.double().requires_grad_(True)
    _, lp = fo.flow_forward(ops, p64, x64, u.double(), [e.double() for e in eps])
    (lp * wts.double()).sum().backward()
    ref = x64.grad
    x32 = x.clone().requires_grad_(True)
    _, lp32 = fo.flow_forward(ops, params, x32, u, eps)
    (lp32 * wts).sum().backward()
    scale = ref.abs().max().item()
    floor = (x32.grad.double() - ref).abs().max().item() / scale
    # product
    model = _frozen(build_model(name, params)).eval()
    set_noise(model, u, eps)
    xd = x.to(DEV).requires_grad_(True)
    z, logp = model(xd)
    assert logp.requires_grad and not z.requires_grad
    (logp * wts.to(DEV)).sum().backward()
    assert xd.grad is not None and xd.grad.shape == xd.shape and xd.grad.dtype == torch.float32
    assert (bpd(logp.detach().cpu(), name) - bpd(lp.detach().float(), name)).abs().max() < BPD_TOL
    grad, logp2 = model.score(x.to(DEV), weights=wts.to(DEV))
    assert torch.equal(grad, xd.grad) and torch.equal(logp2, logp.detach())
    assert all(p.grad is None for p in model.parameters())
    err = (xd.grad.cpu().double() - ref).abs().max().item() / scale
    tol = max(1e-4, 3.0 * floor)
    print("score %s B=%d %s: relative error %.3e, fp32 floor %.3e, bar %.3e" % (name, B, tag, err, floor, tol))
    assert err < tol, "relative input-gradient error %.3e (fp32 floor %.3e, bar %.1e)" % (err, floor, tol)


# ------------------------------------------------------------------------------------------ 2. data-only = training path
@pytest.mark.gpu
@pytest.mark.parametrize("name,B", [("cifar10", 5), ("cifar10", 70), ("cifar10", 1537), ("mnist", 37)])
def test_data_only_walk_equals_the_training_path(L, name, B):
    """x.grad with every parameter trainable (the training backward: operand planes written, side streams at B <= 1024) is
    bitwise x.grad with every parameter frozen (cf_flow_step_bwd_data, no planes); logp too; and asking for x.grad changes no
    parameter gradient.  1537 = one past the batch up to which the 4x4 level runs one sample per workgroup: the tile form with
    a ragged last tile."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e(name)
    x, u, eps, g = _inputs(name, B, 5)
    wts = torch.randn(B, M, generator=g).to(DEV)
    model = build_model(name, params).train()
    set_noise(model, u, eps)

    def run(frozen, xgrad):
        _frozen(model, frozen)
        xd = x.to(DEV).requires_grad_(xgrad)
        _, logp = model(xd)
        (logp * wts).sum().backward()
        torch.cuda.synchronize()
        return xd.grad, logp.detach(), {k: (p.grad.clone() if p.grad is not None else None) for k, p in model.named_parameters()}

    gx_t, lp_t, gp_t = run(False, True)
    gx_f, lp_f, gp_f = run(True, True)
    _, lp_p, gp_p = run(False, False)
    assert gx_t is not None and gx_f is not None
    assert torch.equal(gx_t, gx_f) and torch.equal(lp_t, lp_f) and torch.equal(lp_t, lp_p)
    assert all(v is None for v in gp_f.values())
    assert sum(v is not None for v in gp_t.values()) >= 30
    for k, v in gp_t.items():
        assert (v is None) == (gp_p[k] is None), k
        if v is not None:
            assert torch.equal(v, gp_p[k]), k


# ------------------------------------------------------------------------------------------ 3. no weight-gradient work
@pytest.mark.gpu
def test_score_launches_no_weight_gradient_work(L, monkeypatch):
    from contextflow_amd.layers import _hip
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e("cifar10")
    x, u, eps, g = _inputs("cifar10", 5, 7)
    model = build_model("cifar10", params)         # parameters trainable: score takes the data-only walk all the same
    set_noise(model, u, eps)
    names = []
    real = _hip.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_hip, "call", recording)
    model.score(x.to(DEV))
    torch.cuda.synchronize()
    monkeypatch.undo()
    nsteps = sum(op[0] == "step" for op in model._plans[tuple(x.shape[1:])])
    assert nsteps > 0 and names.count("cf_flow_step_bwd_data") == nsteps and names.count("cf_flow_step_fwd_taped") == nsteps
    assert names.count("cf_preprocess_bwd") == 1
    assert "cf_flow_step_bwd_taped" not in names
    assert not [n for n in names if "wgrad" in n or "param" in n or n == "cf_gmm_bwd_sums"], names


# ------------------------------------------------------------------------------------------ 4. score semantics
@pytest.mark.gpu
def test_score_semantics(L):
    import contextflow_amd as cfa
    from tests.gpu_util import build_model, set_noise
    name, B = "cifar10", 5
    ops, _, M, params, fx = load_e2e(name)
    x, u, eps, g = _inputs(name, B, 11)
    model = build_model(name, params)
    set_noise(model, u, eps)
    flags = [p.requires_grad for p in model.parameters()]
    xd = x.to(DEV)
    eye = torch.eye(M, device=DEV)
    g3, lp3 = model.score(xd, labels=3)
    gw, lpw = model.score(xd, weights=eye[3].expand(B, M).contiguous())
    assert torch.equal(g3, gw) and torch.equal(lp3, lpw)
    assert g3.shape == xd.shape and g3.dtype == torch.float32 and float(g3.abs().max()) > 0.0
    lab = torch.tensor([0, 9, 3, 3, 1])
    gl, _ = model.score(xd, labels=lab)
    gw, _ = model.score(xd, weights=eye[lab.to(DEV)])
    assert torch.equal(gl, gw)
    assert torch.equal(gl[2], g3[2]) and not torch.equal(gl[0], g3[0])
    gm, lpm = model.score(xd)                            # the marginal: w = softmax of the returned logp
    gw, _ = model.score(xd, weights=torch.softmax(lpm, dim=1))
    assert torch.equal(gm, gw) and torch.equal(lpm, lp3)
    with torch.no_grad():
        gn, lpn = model.score(xd)
    assert torch.equal(gn, gm) and torch.equal(lpn, lpm)
    assert not gm.requires_grad and not lpm.requires_grad and xd.grad is None and not xd.requires_grad
    xr = x.to(DEV).requires_grad_(True)                  # an input that requires a gradient keeps its flag and gets no .grad
    gr, _ = model.score(xr)
    assert torch.equal(gr, gm) and xr.grad is None and xr.requires_grad and not gr.requires_grad
    assert [p.requires_grad for p in model.parameters()] == flags and all(p.grad is None for p in model.parameters())
    with pytest.raises(ValueError):
        model.score(xd, labels=3, weights=eye[3].expand(B, M))
    with pytest.raises(ValueError):
        model.score(xd, labels=M)
    with pytest.raises(ValueError):
        model.score(xd, labels=-1)
    with pytest.raises(ValueError):
        model.score(xd, labels=[0, 1, M, 2, 3])
    with pytest.raises(ValueError):
        model.score(xd, labels=[0, 1, 2])
    # the step tables kept between score calls follow the parameters
    from contextflow_amd.layers import Coupling
    cpl = [m for m in model.sequence_modules if isinstance(m, Coupling)][0]
    with torch.no_grad():
        cpl.NN[2].weight.mul_(0.9)
    ga, lpa = model.score(xd, labels=3)
    model.invalidate_caches()
    gb, lpb = model.score(xd, labels=3)
    assert torch.equal(ga, gb) and torch.equal(lpa, lpb) and not torch.equal(ga, g3)
    # specialist flows are out of scope
    sname, ctx, sops, sM, sparams, inp = load_specialist("mnist_eye_cf")
    cfg, ds, MM = cfa.preset_config(sname)
    cfg.update(generalist=False, enc_emb=ctx["enc_emb"], enc_type=ctx.get("enc_type", "uniform"), contextflow=ctx["contextflow"])
    spec = cfa.create_model(cfg, ds, MM, contexts=ctx["contexts"])
    spec.load_state_dict(sparams, strict=True)
    spec = spec.to(DEV).eval()
    with pytest.raises(NotImplementedError):
        spec.score(inp["x"].to(DEV))


# ------------------------------------------------------------------------------------------ 5. layouts
@pytest.mark.gpu
def test_score_layouts_and_noise_forms(L):
    from tests.gpu_util import build_model, set_noise
    name, B = "mnist", 3
    ops, _, M, params, fx = load_e2e(name)
    C, H, W = fo.CONFIGS[name][0]
    x, u, eps, g = _inputs(name, B, 13)
    wts = torch.randn(B, M, generator=g).to(DEV)
    model = _frozen(build_model(name, params)).eval()
    set_noise(model, u, eps)
    g32, lp32 = model.score(x.to(DEV), weights=wts)
    g32b, _ = model.score(x.to(DEV), weights=wts)        # explicit noise: the same call twice
    assert torch.equal(g32, g32b)
    # fp64, non-contiguous: every second column of a twice as wide tensor
    wide = torch.zeros(B, C, H, 2 * W, dtype=torch.float64)
    wide[..., ::2] = x.double()
    xx = wide.to(DEV)[..., ::2].requires_grad_(True)
    assert not xx.is_contiguous() and xx.is_leaf
    _, logp = model(xx)
    (logp * wts).sum().backward()
    assert xx.grad.dtype == torch.float64 and xx.grad.shape == xx.shape
    assert torch.equal(xx.grad.float(), g32) and torch.equal(logp.detach(), lp32)
    g64, _ = model.score(xx.detach(), weights=wts)
    assert g64.dtype == torch.float32 and torch.equal(g64, g32)
    # one sample
    set_noise(model, u[:1], [e[:1] for e in eps])
    g1, lp1 = model.score(x[:1].to(DEV), weights=wts[:1])
    assert torch.equal(g1, g32[:1]) and torch.equal(lp1, lp32[:1])
    # empty batch: shape-correct, no launch failure - both ways
    set_noise(model, None, [])
    x0 = torch.zeros(0, C, H, W, device=DEV)
    g0, lp0 = model.score(x0)
    assert tuple(g0.shape) == (0, C, H, W) and tuple(lp0.shape) == (0, M)
    x0.requires_grad_(True)
    model(x0)[1].sum().backward()
    assert x0.grad is not None and tuple(x0.grad.shape) == (0, C, H, W)
    # in-kernel noise: the same seed twice
    xd = x.to(DEV)
    torch.manual_seed(77)
    ga, lpa = model.score(xd, weights=wts)
    torch.manual_seed(77)
    gb, lpb = model.score(xd, weights=wts)
    torch.manual_seed(78)
    gc, _ = model.score(xd, weights=wts)
    assert torch.equal(ga, gb) and torch.equal(lpa, lpb) and not torch.equal(ga, gc)
    assert torch.isfinite(ga).all() and not torch.equal(ga, g32)
