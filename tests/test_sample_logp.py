"""`return_logp=True` of inverse / decode / sample: the log-density of the point a backward walk produces.

CPU: the definition (the oracle's forward ops along flow_inverse's trace reproduce flow_forward's logp in fp64), its fp32 floors,
and the closed form of cf_postprocess_inv_ld's log-det.  GPU: the flagged inverse-step kernel per geometry and on every fused
step of the fixtures, the flagged tail kernel, the whole chain against the fp64 trace, the device round trip encode -> decode,
`sample`, and the refusals."""
import math
import os
import subprocess
import sys

import pytest
import torch

from oracle import flow_oracle as fo
from tests.helpers import load_e2e
from tests.sample_logp_util import (BPD_TOL, bpd_entries, cast, floors, postprocess_ld_closed_form, problem, walk_logp)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NAMES = ["mnist", "cifar10", "smap"]
REGIMES = [None, "stress", "extreme"]
GEOMETRIES = [(8, 16), (16, 16), (32, 8), (64, 4)]
ALPHA32 = float(torch.tensor(fo.ALPHA, dtype=torch.float32))                     # Normalization keeps its scalars in fp32
S2_32 = float(torch.tensor(1 / (1 - 2 * fo.ALPHA), dtype=torch.float32))


def close(a, b, tol=1e-5):
    """tests/test_gpu_parity.py's `close`, printing the figure it asserts on."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item()
    assert err <= tol * scale, "max err %.3e (scale %.3e)" % (err, scale)
    return err / scale


def chain_bar(name):
    return max(BPD_TOL, 3.0 * floors(name)[2])


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_definition_reproduces_flow_forward_in_fp64(name):
    """(a) The restated walk - forward log-dets at the recovered inputs, halves and z scored by gmm_logprob, the dropped Augment
    channels by std_normal_neg_logq - equals flow_forward's logp on the default fixture: 1e-9 bits/dim per entry."""
    ops, params, z, halves, inputs, logp, D, _ = problem(name)
    x, lp = walk_logp(ops, cast(params, torch.float64), z, halves)
    assert lp.dtype == torch.float64 and tuple(lp.shape) == tuple(logp.shape)
    e = (bpd_entries(lp, D) - bpd_entries(logp, D)).abs().max().item()
    print("%s definition vs flow_forward, fp64: %.2e bits/dim per entry" % (name, e))
    assert e <= 1e-9
    if name != "smap":
        assert torch.equal(x, inputs[0])


@pytest.mark.parametrize("name", NAMES)
def test_fp32_floor_of_the_definition(name):
    """(b) The same restatement in fp32 from the fp64 latents: the floor the device's whole chain is held to (3 x, or 1e-5).  It
    is recomputed here, finite, and below the bar it sets only through the factor 3."""
    lp64, lp32, floor = floors(name)
    print("%s fp32 floor of the walk's logp: %.2e bits/dim per entry (bar of the chain %.2e)" % (name, floor, chain_bar(name)))
    assert torch.isfinite(lp32).all() and math.isfinite(floor) and 0.0 < floor < 1e-3


def test_closed_form_of_the_tail_log_det():
    """(c) ldj_const + sum softplus(y) + softplus(-y) + sum e^2 / 2 + aug_n log(2 pi) / 2 against the oracle's pre-processing in
    fp64: affine_fwd x 2, logit_fwd at the continuous point, std_normal_neg_logq of the Augment noise."""
    g = torch.Generator().manual_seed(11)
    B, C, H, W = 5, 3, 4, 4
    xq = torch.randint(0, 256, (B, C, H, W), generator=g).double() + torch.rand(B, C, H, W, generator=g, dtype=torch.float64)
    e = torch.randn(B, 1, H, W, generator=g, dtype=torch.float64)
    v, l1 = fo.affine_fwd(xq, 0.0, 256.0)
    v, l2 = fo.affine_fwd(v, fo.ALPHA, 1 / (1 - 2 * fo.ALPHA))
    y, l3 = fo.logit_fwd(v)
    ref = l1 + l2 + l3 + fo.std_normal_neg_logq(e).reshape(B)
    got = postprocess_ld_closed_form(y.flatten(1), e.flatten(1), 0.0, 256.0, ALPHA32, S2_32)
    err = ((got - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
    print("closed form of the tail's log-det vs the oracle's pre-processing, fp64: %.2e relative" % err)
    assert err <= 1e-12
    none = postprocess_ld_closed_form(y.flatten(1), e.flatten(1)[:, :0], 0.0, 256.0, ALPHA32, S2_32)
    assert ((none - (l1 + l2 + l3)).abs() / ref.abs().clamp_min(1.0)).max().item() <= 1e-12


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


def conditioner_form(C, H, B):
    from contextflow_amd.layers import _hip
    macs = _hip.lib().cf_flow_step_macs(B, C, H, H, 3)
    form = {40: "direct", 20: "winograd"}[macs // (C * C * H * H)]
    assert form == ("direct" if os.environ.get("CONTEXTFLOW_DIRECT_CONV", "")[:1] == "1" else "winograd")
    return form


def step_modules(L, C, H):
    torch.manual_seed(C * 1000 + 7)
    conv, act, cpl = L.Conv1x1((C, H, H)), L.ActNorm((C, H, H)), L.Coupling(C, kernel_size=(3, 3), padding=(1, 1))
    with torch.no_grad():
        conv.NN.add_(0.1 * torch.randn(C, C))
        act.NN_t.copy_(0.3 * torch.randn(C)); act.NN_logs.copy_(0.2 * torch.randn(C)); act.initialized.fill_(1)
    act._init_done = True
    return conv, act, cpl


def both_steps(flow, z, conv, act, cpl, unsq, pre):
    """(x of cf_flow_step_inv, x and ld of cf_flow_step_inv_ld on ld pre-filled with `pre`, ld of a second flagged launch)."""
    from contextflow_amd.layers.inverse import _inverse_step
    x0 = _inverse_step(flow, z, conv, act, cpl, unsqueeze=unsq)
    ld = pre.clone()
    x1 = _inverse_step(flow, z, conv, act, cpl, unsqueeze=unsq, ld=ld)
    ld2 = pre.clone()
    _inverse_step(flow, z, conv, act, cpl, unsqueeze=unsq, ld=ld2)
    torch.cuda.synchronize()
    return x0, x1, ld, ld2


@pytest.mark.gpu
@pytest.mark.parametrize("C,H", GEOMETRIES)
def test_step_inv_ld_per_geometry(L, C, H):
    """(d) cf_flow_step_inv_ld at B = 1 and 37 (several workgroups, a ragged last one), dense and batch-strided z, with and
    without the folded un-squeeze, ld_acc pre-filled: x bitwise cf_flow_step_inv's, ld = pre-fill + l0 + l1 + l2 of the fp64
    oracle's forward step at the exact input (1e-5 of scale, the forward kernel's bar), two launches the same bits."""
    import contextflow_amd as cfa
    conv, act, cpl = step_modules(L, C, H)
    dist = L.GaussianMixtureDistribution(size=(C, H, H), mixtures=2, components=8)
    flow = cfa.layers.FlowSequential(dist, conv, act, cpl).to(DEV)
    p = {"0." + k: v.detach().double().cpu() for k, v in cpl.state_dict().items()}
    g = torch.Generator().manual_seed(C + H)
    worst = 0.0
    for B in (1, 37):
        x = torch.randn(B, C, H, H, generator=g).double()
        y, l0 = fo.conv1x1_fwd(x, conv.NN.detach().double().cpu())
        y, l1 = fo.actnorm_fwd(y, act.NN_t.detach().double().cpu(), act.NN_logs.detach().double().cpu())
        z, l2 = fo.coupling_fwd(y, p, "0.", (1, 1))
        ref = l0 + l1 + l2
        form = conditioner_form(C, H, B)
        pre = (3.0 * torch.randn(B, generator=g)).to(DEV)
        wide = (50.0 * torch.randn(B, C + 4, H, H, generator=g)).to(DEV)
        zs = wide[:, 4:]
        zs.copy_(z.float())
        assert not zs.is_contiguous() or B == 1
        for zt in (z.float().to(DEV), zs):
            for unsq in (False, True):
                x0, x1, ld, ld2 = both_steps(flow, zt, conv, act, cpl, unsq, pre)
                assert torch.equal(x0, x1) and torch.equal(ld, ld2)
                worst = max(worst, close(ld, pre.cpu().double() + ref, tol=1e-5))
                want = fo.squeeze_inv(x, (2, 2)) if unsq else x
                close(x1, want, tol=1e-5)
        print("step_inv_ld C=%d H=%d B=%d %s: ld worst %.2e of scale (bar 1e-05), x bitwise, repeatable" % (C, H, B, form, worst))


@pytest.mark.gpu
def test_step_inv_ld_direct_form_in_a_child_process():
    """(d) CONTEXTFLOW_DIRECT_CONV=1 is read once per process: the per-geometry test runs once more in ONE fresh child, where the
    dispatch reports the direct form of the 3x3 for every geometry."""
    env = dict(os.environ, CONTEXTFLOW_DIRECT_CONV="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_sample_logp.py"), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           "-k", "test_step_inv_ld_per_geometry"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if " direct: " in ln]
    print("\n".join(lines))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert len(lines) == 2 * len(GEOMETRIES) and not any(" winograd: " in ln for ln in r.stdout.splitlines())


def fused_steps(ops):
    out = []
    for i in range(len(ops) - 2):
        if (ops[i][0], ops[i + 1][0], ops[i + 2][0]) == ("conv1x1", "actnorm", "coupling"):
            out.append((i, i > 0 and ops[i - 1][0] == "squeeze" and tuple(ops[i - 1][2]) == (2, 2)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("tag", REGIMES)
@pytest.mark.parametrize("name", ["cifar10", "mnist"])
def test_step_inv_ld_on_every_fused_step_of_the_fixtures(L, name, tag):
    """(e) The model's own flagged _inverse_step on the fp64 trace's step outputs - default, stress and extreme parameters: x
    bitwise the unflagged kernel's, ld against the three log-dets the fp64 trace recorded for the step (1e-5 of scale)."""
    from tests.gpu_util import build_model
    ops, params, z, halves, inputs, _, _, ldjs = problem(name, tag)
    model = build_model(name, params)
    mods = model.sequence_modules
    steps = fused_steps(ops)
    assert len(steps) == {"cifar10": 12, "mnist": 4}[name]
    B = z.shape[0]
    g = torch.Generator().manual_seed(len(ops))
    for i, sq in steps:
        C, H = inputs[i].shape[1:3]
        ref = ldjs[i] + ldjs[i + 1] + ldjs[i + 2]
        pre = (3.0 * torch.randn(B, generator=g)).to(DEV)
        x0, x1, ld, ld2 = both_steps(model, inputs[i + 3].float().to(DEV), mods[i], mods[i + 1], mods[i + 2], sq, pre)
        assert torch.equal(x0, x1) and torch.equal(ld, ld2)
        e = close(ld, pre.cpu().double() + ref, tol=1e-5)
        print("%s %s step %d C=%d H=%d unsqueeze=%d B=%d %s: ld %.2e of scale %.1f (bar 1e-05)"
              % (name, tag, ops[i][1], C, H, sq, B, conditioner_form(C, H, B), e, max(1.0, ref.abs().max().item())))


def tail_call(fn, z, x, ld, B, n_keep, aug_n, zbs, clamp):
    from contextflow_amd.layers import _hip
    P, st = _hip.p, _hip.stream()
    N = n_keep
    if fn == "ld":
        cst = -N * math.log(256.0) - N * math.log(S2_32)
        _hip.call("cf_postprocess_inv_ld", P(z), P(x), P(ld), B, n_keep, aug_n, zbs, ALPHA32, S2_32, 0.0, 256.0, cst, int(clamp), 0.0, 255.0, st)
    elif clamp:
        _hip.call("cf_postprocess_inv_clamped", P(z), P(x), B, n_keep, zbs, ALPHA32, S2_32, 0.0, 256.0, 0.0, 255.0, st)
    else:
        _hip.call("cf_postprocess_inv", P(z), P(x), B, n_keep, zbs, ALPHA32, S2_32, 0.0, 256.0, st)


@pytest.mark.gpu
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("n_keep,aug_n", [(3072, 0), (3072, 1024), (1024, 0), (1024, 1024), (7, 0), (7, 5)])
def test_postprocess_inv_ld(L, n_keep, aug_n, clamp):
    """(f) cf_postprocess_inv_ld at B = 1, 3, 33, with and without Augment elements behind the kept ones, aligned and with z 4 bytes
    off (the scalar form): x bitwise cf_postprocess_inv[_clamped]'s, ld = pre-fill + the closed form in fp64 (1e-6 of scale, the
    bar test_preprocessing holds the forward log-det to).  Logits out to +-12: pixels outside [0, 255] in front of the clamp."""
    g = torch.Generator().manual_seed(n_keep + aug_n)
    zbs = n_keep + aug_n
    for B in (1, 3, 33):
        for off in (0, 1):
            buf = torch.randn(B * zbs + 4, generator=g)
            zc = buf[off: off + B * zbs].view(B, zbs)
            zc[:, :n_keep] *= 4.0
            zd = buf.to(DEV)[off: off + B * zbs].view(B, zbs)
            assert zd.data_ptr() % 16 == 4 * off
            pre = (3.0 * torch.randn(B, generator=g)).to(DEV)
            x0 = torch.full((B, n_keep), float("nan"), device=DEV)
            x1 = torch.full((B, n_keep), float("nan"), device=DEV)
            ld = pre.clone()
            tail_call("plain", zd, x0, None, B, n_keep, aug_n, zbs, clamp)
            tail_call("ld", zd, x1, ld, B, n_keep, aug_n, zbs, clamp)
            ld2 = pre.clone()
            tail_call("ld", zd, torch.empty_like(x1), ld2, B, n_keep, aug_n, zbs, clamp)
            torch.cuda.synchronize()
            assert torch.equal(x0, x1) and torch.equal(ld, ld2)
            if clamp:
                assert x1.min().item() >= 0.0 and x1.max().item() <= 255.0
            ref = postprocess_ld_closed_form(zc[:, :n_keep].double(), zc[:, n_keep:].double(), 0.0, 256.0, ALPHA32, S2_32)
            # what the kernel added, against the closed form and of ITS scale (the pre-fill may cancel most of it in the sum)
            e = close(ld.cpu().double() - pre.cpu().double(), ref, tol=1e-6)
            print("postprocess_inv_ld n_keep=%d aug_n=%d clamp=%d B=%d offset %d B: ld %.2e of scale %.1f (bar 1e-06), x bitwise"
                  % (n_keep, aug_n, clamp, B, 4 * off, e, max(1.0, ref.abs().max().item())))


def latents_of(z, halves):
    return [h.float().to(DEV) for h in halves] + [z.float().to(DEV)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_whole_chain_logp_against_the_fp64_trace(L, name):
    """(g) decode([halves..., z], return_logp=True) on the fp64 trace of the default fixture: every (b, m) entry within
    max(1e-5, 3 x the fp32 floor of the restated walk) bits/dim of the fp64 logp; x bitwise decode(latents)."""
    from tests.gpu_util import build_model
    ops, params, z, halves, inputs, logp, D, _ = problem(name)
    model = build_model(name, params)
    lat = latents_of(z, halves)
    x0 = model.decode(lat)
    x1, lp = model.decode(lat, return_logp=True)
    assert torch.equal(x0, x1)
    assert lp.dtype == torch.float32 and tuple(lp.shape) == tuple(logp.shape)
    e = (bpd_entries(lp.cpu(), D) - bpd_entries(logp, D)).abs().max().item()
    print("%s decode(return_logp) vs the fp64 trace: %.2e bits/dim per entry (fp32 floor %.2e, bar %.2e)"
          % (name, e, floors(name)[2], chain_bar(name)))
    assert e <= chain_bar(name)
    xi, lpi = model.inverse(lat[-1], return_logp=True) if not halves else (None, None)
    if xi is not None:
        assert torch.equal(xi, x1) and torch.equal(lpi, lp)
    # layer by layer (every layer's own rule: the pre-processing, Augment, Squeeze, Conv1x1, ActNorm, the couplings): the same bar
    model.fused = False
    y0 = model.decode(lat)
    y1, lpl = model.decode(lat, return_logp=True)
    el = (bpd_entries(lpl.cpu(), D) - bpd_entries(logp, D)).abs().max().item()
    print("%s decode(return_logp), layer by layer: %.2e bits/dim per entry (bar %.2e)" % (name, el, chain_bar(name)))
    assert torch.equal(y0, y1) and el <= chain_bar(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cifar10", "mnist"])
def test_round_trip_on_the_device(L, name):
    """(h) 37 random uint8 images, dequantisation noise in [1/64, 63/64]: encode(x) = (latents, logp_enc), and the logp of
    decode(latents, return_logp=True) is within the sum of the two chain bars of logp_enc, per entry; the pixels come back."""
    from tests.gpu_util import build_model, set_noise
    ops, _, _, params, _ = load_e2e(name)
    C, H, W = fo.CONFIGS[name][0]
    B, D = 37, C * H * W
    g = torch.Generator().manual_seed(37 + C)
    x = torch.randint(0, 256, (B, C, H, W), generator=g).float()
    u = 1.0 / 64 + (1.0 - 2.0 / 64) * torch.rand(B, C, H, W, generator=g)
    eps = [torch.randn(B, 1, H, W, generator=g)]
    model = build_model(name, params)
    set_noise(model, u, eps)
    latents, lp_enc = model.encode(x.to(DEV))
    xr, lp_dec = model.decode(latents, return_logp=True)
    e = (bpd_entries(lp_dec.cpu(), D) - bpd_entries(lp_enc.cpu(), D)).abs().max().item()
    print("%s encode -> decode(return_logp) B=%d: %.2e bits/dim per entry (bar %.2e)" % (name, B, e, 2 * chain_bar(name)))
    assert tuple(lp_dec.shape) == tuple(lp_enc.shape) and e <= 2 * chain_bar(name)
    assert torch.equal(xr.cpu(), x)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cifar10", "smap"])
def test_sample_is_the_same_draw_with_the_flag(L, name):
    """(i) Same seed: sample(33) and sample(33, return_logp=True)[0] are equal, and so is what the generator gives next; logp is
    (33, M), finite."""
    from tests.gpu_util import build_model
    _, _, M, params, _ = load_e2e(name)
    model = build_model(name, params)
    torch.manual_seed(5)
    a = model.sample(33)
    na = torch.rand(4, device=DEV)
    torch.manual_seed(5)
    b, lp = model.sample(33, return_logp=True)
    nb = torch.rand(4, device=DEV)
    assert torch.equal(a, b) and torch.equal(na, nb)
    assert tuple(lp.shape) == (33, M) and lp.dtype == torch.float32 and bool(torch.isfinite(lp).all())
    torch.manual_seed(5)
    c, lp2 = model.sample(33, labels=torch.arange(33) % M, temperature=0.7, return_logp=True)
    torch.manual_seed(5)
    assert torch.equal(c, model.sample(33, labels=torch.arange(33) % M, temperature=0.7))
    assert tuple(lp2.shape) == (33, M) and bool(torch.isfinite(lp2).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cifar10", "mnist"])
def test_sample_logp_is_decodes_logp_at_the_chosen_means(L, name):
    """(i) wG = +-60 and temperature 0 (tests/test_conditional_sampling.py): the draw is the chosen components' mean rows, so
    sample(n, labels, temperature=0, return_logp=True)[1] is decode(those rows, clamp=True, return_logp=True)[1] bit for bit."""
    from tests.gpu_util import build_model
    _, _, M, params, _ = load_e2e(name)
    model = build_model(name, params)
    levels = [m.dist for m in model.sequence_modules if isinstance(m, L.SplitPrior)] + [model.dist]
    n = 33
    c = torch.arange(n) % M
    latents = []
    with torch.no_grad():
        for lv, dist in enumerate(levels):
            j = (3 * c + lv + 1) % dist.K
            dist.wG.fill_(-60.0)
            dist.wG[c, j] = 60.0
            latents.append(dist.mG.detach()[c, j].clone())
    xs, lps = model.sample(n, labels=c, temperature=0.0, return_logp=True)
    xd, lpd = model.decode(latents, clamp=True, return_logp=True)
    assert torch.equal(xs, xd) and torch.equal(xs, model.sample(n, labels=c, temperature=0.0))
    assert tuple(lps.shape) == (n, M) and bool(torch.isfinite(lps).all())
    assert torch.equal(lps, lpd)


@pytest.mark.gpu
def test_refusals(L):
    """(j) A specialist flow and a flow holding an activation layer raise NotImplementedError with return_logp=True; without the
    flag the activation flow still inverts."""
    import contextflow_amd as cfa
    from tests import specialist_inverse_util as su
    p = su.problem("mnist_eye_cf")
    model = su.build_specialist(p)
    lat = [h.float().to(DEV) for h in p.halves] + [p.z.float().to(DEV)]
    ctx = p.context.to(DEV)
    with pytest.raises(NotImplementedError):
        model.decode(lat, context=ctx, return_logp=True)
    with pytest.raises(NotImplementedError):
        model.sample(p.z.shape[0], context=ctx, return_logp=True)
    with pytest.raises(NotImplementedError):
        model.inverse(lat[-1], context=ctx, return_logp=True)
    dist = L.GaussianMixtureDistribution(size=(4, 2, 2), mixtures=2, components=8)
    flow = cfa.layers.FlowSequential(dist, L.Conv1x1((4, 2, 2)), L.LeakyRelu(0.1)).to(DEV)
    z = torch.randn(3, 4, 2, 2, device=DEV)
    assert tuple(flow.inverse(z).shape) == (3, 4, 2, 2)
    with pytest.raises(NotImplementedError, match="LeakyRelu"):
        flow.inverse(z, return_logp=True)
    flow2 = cfa.layers.FlowSequential(dist, L.Conv1x1((4, 2, 2))).to(DEV)
    x, lp = flow2.inverse(z, return_logp=True)
    _, ref = flow2(x)
    assert tuple(lp.shape) == (3, 2) and (lp - ref).abs().max().item() <= 1e-4 * max(1.0, ref.abs().max().item())
