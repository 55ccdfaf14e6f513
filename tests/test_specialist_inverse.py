"""The specialist (context-conditioned) flows backwards: cf_affine_ctx_inv, the context `reverse` of Conv1x1 / ActNorm, pinned
encoder noise (`context_noise`, `noise=`), `inverse` / `encode` / `decode` / `sample` under a context, and cf_gmm_ctx_draw.

The exact answer of an inverse is the fp64 oracle's FORWARD trace (oracle.flow_oracle.inverse_problem); the floor is a test-local
torch restatement of the inverse (tests/specialist_inverse_util.py: per-sample matrix as oracle.conv1x1_ctx_fwd, torch.linalg.solve)
run in fp32 on the CPU on the same operands.  Errors are in units of the reference tensor's scale, max(1, max|ref|).

Whole-chain bars exist only where the reference's own fp32 arithmetic can meet them (CHAIN_FIXTURES: per-sample matrices of
condition <= 26).  cifar10_onehot_cf / smap_onehot_cf / atm_onehot_cf reach conditions of 7.6e3 / 2.3e2 / 9.0e3, a plain fp32
restatement of their whole chain returns garbage; they are held one step at a time (test_every_context_pair_of_the_fixtures)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import flow_oracle as fo
from tests import specialist_inverse_util as U
from tests.helpers import bpd

DEV = U.DEV
ACT_TOL = 1e-5
CHAIN_FLOOR = 2e-5                # the fp32 restatement of the whole chain on CHAIN_FIXTURES (measured: at most 1.3e-5)
BPD_TOL = 1e-5
SHAPES = [(16, 16, 16), (32, 8, 8), (64, 4, 4), (8, 16, 16), (26, 8, 1), (76, 18, 1), (76, 12, 12)]


@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


# ------------------------------------------------------------------------------------------ 1. CPU: the floors
@pytest.mark.parametrize("fxname", U.CHAIN_FIXTURES)
def test_fp32_floor_of_the_chain_and_the_pixels(fxname):
    """The fact the GPU bars rest on: with the dequantisation noise at 0.5 the fp32 restatement of the inverse chain stays
    within 2e-5 of scale of the fp64 trace in front of the pre-processing and, continued through it, flips no pixel.
    Measured: mnist_eye_cf 1.9e-6, mnist_onehot 5.6e-6, cifar10_eye 1.4e-6, cifar10_eye_vardeq_cf 4.1e-6, cifar10_embed_eyesample
    1.0e-6, mnist_embed_probsample_cf 2.7e-6, cifar10_eye_argmax_cf 1.3e-5."""
    p = U.problem(fxname, 4, True)
    e, pix = U.chain_floor(fxname, 4, True)
    wrong = int((pix != p.x).sum())
    print("%s: fp32 chain %.2e of scale (bar %.0e), %d of %d pixels wrong" % (fxname, e, CHAIN_FLOOR, wrong, p.x.numel()))
    assert e <= CHAIN_FLOOR
    assert wrong == 0


# ------------------------------------------------------------------------------------------ 2. the noise object
@pytest.mark.gpu
@pytest.mark.parametrize("fxname", ["cifar10_onehot_cf", "mnist_embed_probsample_cf", "cifar10_embed_eyesample"])
def test_context_noise_has_one_tensor_per_stochastic_encoder(L, fxname):
    """`context_noise(context)`: one device tensor per UniformCatDequantization / ConditionalGaussianDistribution in modules()
    order, in the shapes the fixture's recorded encoder noise has (none for the embedding lookup); `noise=` pins them for the
    call alone and leaves an encoder the caller pinned alone; a wrong count or shape is a ValueError."""
    p = U.problem(fxname, 4)
    model = U.build_specialist(p)
    cd = p.context.to(DEV)
    n = model.context_noise(cd)
    encs = model._stochastic_encoders()
    assert len(n) == len(n.tensors) == len(encs) == len(p.cnoise)
    for t, c, e in zip(n, p.cnoise, encs):
        assert tuple(t.shape) == tuple(c.shape) and t.dtype == torch.float32 and t.device == torch.device(DEV)
        assert isinstance(e, (L.UniformCatDequantization, L.ConditionalGaussianDistribution))
        if isinstance(e, L.UniformCatDequantization):
            assert 0.0 <= float(t.min()) and float(t.max()) < 1.0
    z = p.z.float().to(DEV)
    lat = [h.float().to(DEV) for h in p.halves] + [z]
    a = model.decode(lat, cd, noise=n)
    assert all(e.fixed_noise is None for e in encs)
    assert torch.equal(a, model.decode(lat, cd, noise=n))
    if encs:
        assert not torch.equal(a, model.decode(lat, cd))                   # fresh codes without it
        mine = torch.full_like(n.tensors[0], 0.25)
        encs[0].fixed_noise = mine
        try:
            b = model.decode(lat, cd, noise=n)
            assert encs[0].fixed_noise is mine
        finally:
            encs[0].fixed_noise = None
        assert torch.equal(b, model.decode(lat, cd, noise=[mine] + n.tensors[1:]))
        with pytest.raises(ValueError):
            model.decode(lat, cd, noise=n.tensors[:-1])
        with pytest.raises(ValueError):
            model.decode(lat, cd, noise=[t[:2] for t in n.tensors])
        with pytest.raises(ValueError):
            model.decode(lat, cd, noise=n.tensors[:-1] + [n.tensors[-1][:2]])
    for call in (lambda: model.decode(lat), lambda: model.inverse(z), lambda: model.encode(p.x.to(DEV)), lambda: model.sample(4)):
        with pytest.raises(ValueError, match="context"):
            call()


# ------------------------------------------------------------------------------------------ 3. the kernel alone
def _inv_call(z, m1, Wm, m2, t, logs, out, B, C, H, W, zbs, unsq):
    from contextflow_amd.layers import _hip
    P = _hip.p
    _hip.call("cf_affine_ctx_inv", P(z), P(m1), P(Wm), P(m2), P(t), P(logs), P(out), B, C, H, W, zbs, unsq, _hip.stream())


def _operands(C, H, W, B, g, m1_scale):
    r = lambda *sh: torch.randn(*sh, generator=g)
    z, m1, m2 = r(B, C, H, W), m1_scale * r(B, C * C), 0.3 * r(B, 2 * C)
    Wm, logs, t = torch.linalg.qr(r(C, C))[0].contiguous(), 0.2 * r(C), 0.5 * r(C)
    return z, m1, m2, Wm, logs, t, r


@pytest.mark.gpu
@pytest.mark.parametrize("C,H,W", SHAPES)
def test_affine_ctx_inv_against_fp64(L, C, H, W):
    """cf_affine_ctx_inv: x = W_b^-1 (z exp(l_b) + t_b) against the fp64 formula at the three image levels, mnist's level, SMAP's 26
    and ATM's 76 channels (the last above 64 KiB of LDS); B in {1, 5, 9}; with and without Wm / t / logs; m1 = NULL; m2 = NULL;
    out_unsqueeze where C % 4 == 0 (bitwise squeeze_op(..., reverse) of the plain result); a batch-strided z; a z 4 bytes off
    16-byte alignment; sentinels behind x_out; B = 0.  Operands of test_affine_ctx_bwd_data_against_fp64 with m1 = 0.1 randn
    (condition at most 12, fp32 floor at most 1.1e-6): bar 2e-5 max(1, max|ref|), the forward twin's.  One harder pass with m1 =
    0.3 randn (condition up to 2.6e3, floor up to 1.5e-5): bar max(2e-5, 3 x the floor the test computes).
    Measured on an MI355X: at most 0.006 of the bar on the 0.1 operands at every shape; the harder pass under contextflow 1.5e-7,
    2.6e-7, 7.6e-7, 1.4e-7, 2.4e-7, 6.8e-6, 7.0e-6 of scale over the seven shapes against floors of 5.4e-7, 1.5e-6, 1.2e-5, 2.7e-7,
    1.4e-6, 1.7e-5, 3.1e-5 (the kernel refines its solution once with an fp64 residual; without that step: 7.0e-5 at (76,18,1))."""
    from contextflow_amd.layers import _hip
    from contextflow_amd.layers.squeeze import squeeze_op
    g = torch.Generator().manual_seed(C * 131 + H)
    n, PAD, worst = C * H * W, 64, 0.0
    d = lambda v: None if v is None else v.to(DEV).contiguous()
    for B in (1, 5, 9):
        z, m1, m2, Wm, logs, t, r = _operands(C, H, W, B, g, 0.1)
        wide = torch.cat([z, r(B, C, H, W)], 1).to(DEV)                      # z as a channel slice: batch stride 2 C H W
        flat = torch.zeros(B * n + 4, device=DEV)
        flat[1:1 + B * n] = z.reshape(-1).to(DEV)
        layouts = {"dense": (z.to(DEV), n), "strided": (wide[:, :C], 2 * n), "misaligned": (flat[1:1 + B * n].view(B, C, H, W), n)}
        assert layouts["misaligned"][0].data_ptr() % 16 == 4
        for cf in (True, False):
            for half in ("both", "conv", "act"):
                a1, aW = (m1, Wm if cf else None) if half != "act" else (None, None)
                a2, at, al = (m2, t if cf else None, logs if cf else None) if half != "conv" else (None, None, None)
                ref = U.affine_inv_ref(z, a1, aW, a2, at, al)
                bar = 2e-5 * max(1.0, ref.abs().max().item())
                plain = None
                for lay, (zv, zbs) in layouts.items():
                    for unsq in ((0, 1) if C % 4 == 0 else (0,)):
                        if lay != "dense" and (unsq or half != "both"):
                            continue
                        buf = torch.full((B * n + PAD,), -77.0, device=DEV)
                        _inv_call(zv, d(a1), d(aW), d(a2), d(at), d(al), buf, B, C, H, W, zbs, unsq)
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
    print("cf_affine_ctx_inv (%d,%d,%d): worst error / bar %.3f" % (C, H, W, worst))
    # the harder pass
    B = 5
    z, m1, m2, Wm, logs, t, _ = _operands(C, H, W, B, g, 0.3)
    for cf in (True, False):
        aW, at, al = (Wm, t, logs) if cf else (None, None, None)
        ref = U.affine_inv_ref(z, m1, aW, m2, at, al)
        sc = max(1.0, ref.abs().max().item())
        floor = (U.affine_inv_ref(z, m1, aW, m2, at, al, torch.float32).double() - ref).abs().max().item() / sc
        bar = max(2e-5, 3.0 * floor)
        out = torch.empty(B, C, H, W, device=DEV)
        _inv_call(z.to(DEV), d(m1), d(aW), d(m2), d(at), d(al), out, B, C, H, W, n, 0)
        err = (out.cpu().double() - ref).abs().max().item() / sc
        print("cf_affine_ctx_inv (%d,%d,%d) m1 = 0.3 randn, contextflow %d: %.2e of scale, fp32 floor %.2e, bar %.2e" % (C, H, W, cf, err, floor, bar))
        assert err <= bar, (cf, err, floor, bar)
    N = _hip.p(None)
    assert _hip.lib().cf_affine_ctx_inv(N, N, N, N, N, N, N, 0, C, H, W, n, 0, N) == 0


# ------------------------------------------------------------------------------------------ 4. kernel round trip
@pytest.mark.gpu
@pytest.mark.parametrize("C,H,W", SHAPES)
def test_affine_ctx_round_trip(L, C, H, W):
    """cf_affine_ctx_inv(cf_affine_ctx_fwd(x)) returns x to 1e-5 of scale on the seven shapes with the m1 = 0.1 randn operands, with
    and without Wm / t / logs, in_squeeze / out_unsqueeze paired where C % 4 == 0."""
    from contextflow_amd.layers import _hip
    P, st = _hip.p, _hip.stream()
    g = torch.Generator().manual_seed(C * 17 + W)
    B = 5
    x, m1, m2, Wm, logs, t, _ = (v.to(DEV) if torch.is_tensor(v) else v for v in _operands(C, H, W, B, g, 0.1))
    for cf in (True, False):
        aW, at, al = (Wm, t, logs) if cf else (None, None, None)
        for sq in ((0, 1) if C % 4 == 0 else (0,)):
            xin = x.view(B, C // 4, 2 * H, 2 * W) if sq else x               # (the un-squeezed layout of the same numbers)
            zf = torch.empty(B, C, H, W, device=DEV)
            ldj = torch.empty(B, device=DEV)
            _hip.call("cf_affine_ctx_fwd", P(xin), P(m1), P(aW), P(m2), P(at), P(al), None, 0.0, P(zf), P(ldj), B, C, H, W, C * H * W, sq,
                      0, 0, st)
            back = torch.empty_like(xin)
            _inv_call(zf, m1, aW, m2, at, al, back, B, C, H, W, C * H * W, sq)
            e = U.err_of(back, xin)
            print("affine round trip (%d,%d,%d) contextflow %d squeeze %d: %.2e of scale (bar %.0e)" % (C, H, W, cf, sq, e, ACT_TOL))
            assert e <= ACT_TOL, (cf, sq, e)


# ------------------------------------------------------------------------------------------ 5. every per-sample step
@pytest.mark.gpu
@pytest.mark.parametrize("fxname", U.STEP_FIXTURES)
def test_every_context_pair_of_the_fixtures(L, fxname, monkeypatch):
    """Every context Conv1x1 / ActNorm pair of all eleven fixtures is fed the fp64 trace's step output and must return the trace's
    step input - as ONE cf_affine_ctx_inv launch (with the Squeeze((2,2)) in front of it where the walk pairs it) and as two
    `reverse` calls.  Bar per step: max(1e-5, 3 x the fp32 floor of that step) of scale: 1e-5 everywhere but on cifar10_onehot_cf /
    atm_onehot_cf (condition 7.6e3 / 9.0e3: about 7e-4 where the measuring machine's fp32 solve loses 2.3e-4).
    Measured on an MI355X, worst step (fp32 floor): mnist_eye_cf 7.7e-8 (1.7e-7), mnist_onehot 4.6e-7 (6.5e-7), cifar10_eye 1.7e-7
    (1.7e-7), cifar10_eye_vardeq_cf 9.3e-8 (3.6e-7), cifar10_embed_eyesample 1.3e-7 (1.4e-7), mnist_embed_probsample_cf 1.9e-7
    (6.6e-7), cifar10_eye_argmax_cf 1.3e-7 (8.0e-7), cifar10_onehot_cf 1.9e-6 (6.0e-6), smap_onehot_cf 7.4e-7 (8.8e-7), smap_eye
    1.1e-7 (6.8e-8), atm_onehot_cf 1.2e-5 (2.0e-5)."""
    from contextflow_amd.layers import _hip
    from contextflow_amd.layers.conv1x1 import affine_ctx_inverse
    from contextflow_amd.layers.squeeze import squeeze_op
    p = U.problem(fxname, 4)
    model = U.build_specialist(p)
    mods = model.sequence_modules
    p32 = U.cast(p.params, torch.float32)
    code = U.codes(p.ops, p32, p.ctx, p.context, p.cnoise, torch.float32)
    cd = p.context.to(DEV)
    pairs = U.ctx_pairs(p.ops)
    assert pairs
    names = []
    real = _hip.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    worst = (0.0, 0.0, 0.0, 0.0)                    # (error / bar, error, floor, bar) of the step closest to its bar
    with model._pinned(U.fixture_noise(p), cd):
        for i, sq in pairs:
            conv, act = mods[p.ops[i][1]], mods[p.ops[i + 1][1]]
            assert isinstance(conv, L.Conv1x1) and isinstance(act, L.ActNorm) and conv.context_net and act.context_net
            zin, want = p.inputs[i + 2], p.inputs[i - 1] if sq else p.inputs[i]
            y = U.ctx_op_inverse(p.ops[i], p32, p.ctx, code[i], U.ctx_op_inverse(p.ops[i + 1], p32, p.ctx, code[i + 1], zin.float()))
            floor = U.err_of(fo.squeeze_inv(y, (2, 2)) if sq else y, want)
            bar = max(ACT_TOL, 3.0 * floor)
            zd = zin.float().to(DEV)
            monkeypatch.setattr(_hip, "call", recording)
            del names[:]
            one = affine_ctx_inverse(zd, conv=conv, act=act, context=cd, unsqueeze=sq)
            assert names.count("cf_affine_ctx_inv") == 1 and "cf_squeeze" not in " ".join(names)
            monkeypatch.undo()
            two = conv.reverse(act.reverse(zd, cd), cd)
            if sq:
                two = squeeze_op(two, (2, 2), True)
            e1, e2 = U.err_of(one, want), U.err_of(two, want)
            worst = max(worst, (max(e1, e2) / bar, max(e1, e2), floor, bar))
            assert e1 <= bar and e2 <= bar, (p.ops[i][1], sq, e1, e2, floor, bar)
    print("%s: %d pairs, worst step %.2e of scale (fp32 floor %.2e, bar %.2e)" % ((fxname, len(pairs)) + worst[1:]))


# ------------------------------------------------------------------------------------------ 6. whole chain
@pytest.mark.gpu
@pytest.mark.parametrize("B", [4, 9])
@pytest.mark.parametrize("fxname", U.CHAIN_FIXTURES)
def test_whole_chain_against_the_fp64_trace(L, fxname, B, monkeypatch):
    """`inverse(z, context, noise=)` on the flow behind the pre-processing, the fixture's encoder noise pinned and the trace's split
    halves put back, against the trace's tensor there: max(1e-5, 3 x the fp32 floor of the chain) of scale; B = 9 (rows
    0,1,2,3,0,1,2,3,1).  Every ActNorm(c) <- Conv1x1(c) pair is one cf_affine_ctx_inv launch and no Squeeze in front of a pair runs on
    its own.
    Measured on an MI355X, B = 4 and 9 alike (fp32 floor): mnist_eye_cf 2.4e-7 (8.4e-7), mnist_onehot 4.1e-6 (4.6e-6), cifar10_eye
    5.8e-7 (7.0e-7), cifar10_eye_vardeq_cf 4.4e-7 (2.9e-6), cifar10_embed_eyesample 4.2e-7 (4.9e-7), mnist_embed_probsample_cf
    6.0e-7 (1.5e-6), cifar10_eye_argmax_cf 9.2e-7 (5.2e-6)."""
    from contextflow_amd.layers import _hip
    from tests.gpu_util import set_split_draws
    p = U.problem(fxname, B)
    floor, _ = U.chain_floor(fxname, B)
    bar = max(ACT_TOL, 3.0 * floor)
    model = U.build_specialist(p)
    sub = L.FlowSequential(model.dist, *model.sequence_modules[p.first:])
    cd = p.context.to(DEV)
    names = []
    real = _hip.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_hip, "call", recording)
    with set_split_draws(model, [h.float() for h in p.halves]):
        got = sub.inverse(p.z.float().to(DEV), cd, noise=U.fixture_noise(p))
    monkeypatch.undo()
    pairs = U.ctx_pairs(p.ops)
    assert names.count("cf_affine_ctx_inv") == len(pairs)
    assert names.count("cf_squeeze") == sum(o[0] == "squeeze" for o in p.ops) - sum(sq for _, sq in pairs)
    e = U.err_of(got, p.inputs[p.first])
    print("%s chain B=%d: %.2e of scale (fp32 floor %.2e, bar %.2e)" % (fxname, B, e, floor, bar))
    assert e <= bar


# ------------------------------------------------------------------------------------------ 7. pixel cycle
@pytest.mark.gpu
@pytest.mark.parametrize("fxname", U.CHAIN_FIXTURES)
def test_pixel_cycle_and_encode(L, fxname):
    """Dequantisation noise 0.5, the fixture's encoder noise as `noise=`: decode(encode(x, c, noise=n), c, noise=n) returns every
    pixel; encode's logp is within the bits/dim bar of the fp64 oracle's, its latents within 1e-5 of scale of the trace."""
    p = U.problem(fxname, 4, True)
    model = U.build_specialist(p, p.u, p.eps)
    xd, cd, n = p.x.to(DEV), p.context.to(DEV), U.fixture_noise(p)
    lat, logp = model.encode(xd, cd, noise=n)
    assert len(lat) == len(p.halves) + 1 and tuple(logp.shape) == (4, p.M)
    for got, want in zip(lat, p.halves + [p.z]):
        e = U.err_of(got, want)
        assert got.is_contiguous() and e <= ACT_TOL, (fxname, tuple(want.shape), e)
    btol = max(BPD_TOL, 1e-5 * bpd(p.lp.float(), p.name).abs().max().item())
    berr = (bpd(logp.cpu(), p.name) - bpd(p.lp.float(), p.name)).abs().max().item()
    back = model.decode(lat, cd, noise=n)
    wrong = int((back.cpu() != p.x).sum())
    print("%s pixel cycle: %d of %d pixels wrong; bits/dim error %.2e (bar %.1e)" % (fxname, wrong, p.x.numel(), berr, btol))
    assert berr < btol
    assert tuple(back.shape) == tuple(p.x.shape) and back.dtype == torch.float32
    assert wrong == 0


# ------------------------------------------------------------------------------------------ 8. cf_gmm_ctx_draw
def _ctx_draw_call(mG, sG, cdf, c, labels, label0, u, eps, z1, zbs, D1, out, B, M, K, D, HW, T):
    from contextflow_amd.layers import _hip
    P = _hip.p
    _hip.call("cf_gmm_ctx_draw", P(mG), P(sG), P(cdf), P(c), P(labels), label0, P(u), P(eps), None, 0, P(z1), zbs, D1, P(out), B, M, K, D,
              HW, T, _hip.stream())
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("D,HW", [(2048, 16), (96, 1), (96, 6), (7, 7), (7, 1)])
def test_ctx_draw_kernel_with_explicit_noise(L, D, HW):
    """cf_gmm_ctx_draw, u and eps given: (M, K) = (3, 5), D in {2048, 96, 7} (channels of 16 / 1 / 6 / 7 / 1 pixels: shifts that
    change inside a float4), D1 in {0, D, 3}, B in {1, 3, 1001, 0}, T in {1, 0.7, 0}.  Upper half against (mG + cm_b) + T softplus(sG
    + cs_b) eps in fp64: 1e-6 of max(1, |out|); lower half bitwise z1; sentinels around the output; every operand in turn 4 bytes
    off a 16-byte boundary gives the bits of the aligned run; c = 0 is bitwise cf_gmm_draw; T = 0 returns fl(mG + cm_b) exactly.
    Operand scales: the kernel rounds sG + cs_b to fp32 before the softplus, half an ulp of the sum times |eps| <= 4.5 in the
    output; the pre-softplus sums stay inside (-4, 4) here - sG in [-3, 3], shifts 0.25 randn clamped to 0.9 - where that is
    1.2e-7 x 4.5, inside the bar (with sums in [4, 8) the ulp alone would spend all of it)."""
    from tests.test_conditional_sampling import cdf_tables, close, draw_call, frame_intact, framed, pick_uniforms, shifted
    M, K, Dch = 3, 5, D // HW
    g = torch.Generator().manual_seed(3000 + D + HW)
    mG = (3.0 * torch.randn(M * K, D, generator=g)).to(DEV)
    sG = (6.0 * torch.rand(M * K, D, generator=g) - 3.0).to(DEV)            # |sG + cs_b| < 4 (see the docstring)
    wG = 2.0 * torch.rand(M, K, generator=g) - 1.0
    c64, c32 = cdf_tables(wG)
    cdf = c32.to(DEV)
    worst = 0.0
    for B in (1, 3, 1001, 0):
        lab = torch.randint(0, M, (max(B, 1),), generator=g)
        lab[0], lab[-1] = 0, M - 1
        lab = lab[:B]
        u, k = pick_uniforms(c64, lab, g)
        eps = torch.randn(B, D, generator=g)
        c = (0.25 * torch.randn(B, 2, M * K, Dch, generator=g)).clamp(-0.9, 0.9)
        rows = lab * K + k
        ar = torch.arange(B)
        cm = c[ar, 0, rows].repeat_interleave(HW, dim=1)                       # (B, D): constant over the pixels of a channel
        cs = c[ar, 1, rows].repeat_interleave(HW, dim=1)
        base = mG.cpu().double()[rows] + cm.double()
        spread = F.softplus(sG.cpu().double()[rows] + cs.double()) * eps.double()
        mean32 = mG.cpu()[rows] + cm                                           # fl(mG + cm_b)
        lab_d, u_d, eps_d, c_d = lab.to(DEV, torch.int32), u.to(DEV), eps.to(DEV), c.reshape(B, 2 * M * K * Dch).to(DEV)
        for D1 in (0, D, 3):
            W = D1 + D
            z1 = torch.randn(B, D1, generator=g).to(DEV) if D1 else None
            for T in (1.0, 0.7, 0.0):
                ref = base + T * spread
                buf, out = framed(B, W)
                _ctx_draw_call(mG, sG, cdf, c_d, lab_d, 0, u_d, eps_d, z1, D1, D1, out, B, M, K, D, HW, T)
                assert frame_intact(buf, B, W), (B, D1, T)
                e = close(out[:, D1:], ref)
                worst = max(worst, e)
                assert e <= 1e-6, (B, D1, T, e)
                if D1:
                    assert torch.equal(out[:, :D1], z1), (B, D1, T)
                if T == 0.0 and B:
                    assert torch.equal(out[:, D1:].cpu(), mean32)
                if B == 0 or T != 0.7:
                    continue
                plain, ctx0 = torch.empty(B, W, device=DEV), torch.empty(B, W, device=DEV)
                draw_call(mG, sG, cdf, lab_d, 0, u_d, eps_d, None, 0, z1, D1, D1, plain, B, M, K, D, T)
                _ctx_draw_call(mG, sG, cdf, torch.zeros_like(c_d), lab_d, 0, u_d, eps_d, z1, D1, D1, ctx0, B, M, K, D, HW, T)
                assert torch.equal(plain, ctx0), (B, D1, "c = 0")
                for which in ("mG", "sG", "eps", "z1", "out", "c"):
                    if which == "z1" and not D1:
                        continue
                    a = dict(mG=mG, sG=sG, eps=eps_d, z1=z1, c=c_d)
                    if which != "out":
                        a[which] = shifted(a[which])
                    off = 1 if which == "out" else 0
                    buf2, out2 = framed(B, W, off)
                    _ctx_draw_call(a["mG"], a["sG"], cdf, a["c"], lab_d, 0, u_d, a["eps"], a["z1"], D1, D1, out2, B, M, K, D, HW, T)
                    assert frame_intact(buf2, B, W, off), (B, D1, which)
                    assert torch.equal(out2, out), (B, D1, which)
    print("cf_gmm_ctx_draw D=%d HW=%d: worst error %.2e of max(1, |out|) (bar 1e-06)" % (D, HW, worst))


# ------------------------------------------------------------------------------------------ 9. sample under a context
def _mixture_levels(L, model):
    return [m.dist for m in model.sequence_modules if isinstance(m, L.SplitPrior)] + [model.dist]


@pytest.mark.gpu
@pytest.mark.parametrize("fxname", ["cifar10_onehot_cf", "mnist_eye_cf"])
def test_sample_under_a_context(L, fxname):
    """sample(n, context, noise=): finite pixels in [0, 255] of the right shape, repeatable under a seed.  One component per class
    carries all the weight at every level (wG = +-60: the cdf is exactly 0 / 1) and T = 0: sample equals decode(clamp=True) of
    the context-shifted mean rows fl(mG + cm_b), bit for bit - the shift of every sample arrived at every level.  Two different
    contexts give different images; a specialist flow without a context raises ValueError."""
    p = U.problem(fxname, 4)
    model = U.build_specialist(p)
    M = p.M
    n = 2 * M
    card = p.ctx["contexts"]
    g = torch.Generator().manual_seed(7)
    ctx = torch.stack([torch.randint(0, k, (n,), generator=g) for k in card], 1).to(DEV)
    ctx2 = torch.stack([(ctx[:, j] + 1) % k for j, k in enumerate(card)], 1)
    noise = model.context_noise(ctx)
    torch.manual_seed(11)
    a = model.sample(n, ctx, noise=noise)
    torch.manual_seed(11)
    b = model.sample(n, ctx, noise=noise)
    assert tuple(a.shape) == (n,) + tuple(fo.CONFIGS[p.name][0]) and a.dtype == torch.float32
    assert bool(torch.isfinite(a).all()) and float(a.min()) >= 0.0 and float(a.max()) <= 255.0 and torch.equal(a, a.floor())
    assert torch.equal(a, b)
    levels = _mixture_levels(L, model)
    assert all(d.context_net for d in levels)
    c = torch.arange(n) % M
    latents = []
    with torch.no_grad():
        for lv, dist in enumerate(levels):
            j = (3 * c + lv + 1) % dist.K
            dist.wG.fill_(-60.0)
            dist.wG[c, j] = 60.0
            cdf = dist.component_cdf()
            assert bool(((cdf == 0) | (cdf == 1)).all())
            Dch = dist.mG.shape[2]
            shifts = dist.context_net(ctx)[0].reshape(n, 2, dist.M, dist.K, Dch)
            cm = shifts[torch.arange(n), 0, c.to(DEV), j.to(DEV)]
            assert float(cm.abs().max()) > 0.0
            latents.append(dist.mG.detach()[c, j] + cm[:, :, None, None])
    got = model.sample(n, ctx, labels=c, temperature=0.0, noise=noise)
    want = model.decode(latents, ctx, clamp=True, noise=noise)
    assert torch.equal(got, want)
    other = model.sample(n, ctx2, labels=c, temperature=0.0, noise=noise)
    assert not torch.equal(got, other)
    with pytest.raises(ValueError, match="context"):
        model.sample(n)
    with pytest.raises(ValueError):
        model.sample(n + 1, ctx)
