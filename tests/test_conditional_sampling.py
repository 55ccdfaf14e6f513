"""Class-conditional, tempered sampling and the exact encode / decode pair.

CPU (unmarked): the cumulative component table `GaussianMixtureDistribution.component_cdf` against fp64.

GPU (-m gpu): cf_gmm_draw with explicit noise against the fp64 formula (both forms of the kernel, every operand 4 bytes
off, a batch-strided kept half, sentinels around the output), its in-kernel Philox noise (component frequencies, moments,
repeatability, independence of the temperature), `GaussianMixtureDistribution.sample(labels=, temperature=)`, and on the
cifar10 / mnist fixtures `FlowSequential.sample(labels=, temperature=)`, `encode` against the fp64 oracle trace and
`decode(encode(x))` returning every pixel.

Rounding order of the kernel (include/contextflow_hip.h): ts = fl(temperature * softplus(sG)), out = fma(ts, eps, mG) - the
arithmetic of cf_gmm_sample with one more fp32 multiply, held to the same 1e-6 of max(1, |out|)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import flow_oracle as fo
from tests.helpers import load_e2e

DEV = "cuda:0"
ACT_TOL = 1e-5                    # activations against fp64, of the tensor's scale (tests/test_sampling.py)
SENT = 12345.0
PAD = 8                           # sentinel floats on either side of an output: 32 bytes, the output stays 16-byte aligned


def cdf_tables(wG):
    """(fp64 cumulative softmax, the fp32 table the kernel reads: rounded once, last column exactly 1)."""
    c64 = torch.cumsum(torch.softmax(wG.double(), dim=-1), dim=-1)
    c32 = c64.float()
    c32[:, -1] = 1.0
    return c64, c32


# ---- CPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(3, 5), (10, 8)])
def test_component_cdf_against_fp64(M, K):
    """component_cdf() on a host module: monotone in k, last column exactly 1.0, within 1e-7 of the fp64 cumulative softmax
    (one fp32 rounding of a number <= 1 is at most 6e-8); kept while wG is unchanged, rebuilt after an in-place update."""
    import contextflow_amd as cfa
    g = torch.Generator().manual_seed(M * 100 + K)
    dist = cfa.layers.GaussianMixtureDistribution(size=(2, 1, 1), mixtures=M, components=K)
    with torch.no_grad():
        dist.wG.copy_(2.0 * torch.rand(M, K, generator=g) - 1.0)
    cdf = dist.component_cdf()
    c64, _ = cdf_tables(dist.wG.detach())
    assert tuple(cdf.shape) == (M, K) and cdf.dtype == torch.float32 and cdf.is_contiguous()
    assert torch.all(cdf[:, 1:] >= cdf[:, :-1]) and torch.all(cdf[:, 0] > 0)
    assert torch.all(cdf[:, -1] == 1.0)
    err = (cdf.double() - c64).abs().max().item()
    print("component_cdf M=%d K=%d: %.2e from fp64 (bar 1e-07)" % (M, K, err))
    assert err <= 1e-7
    assert dist.component_cdf() is cdf
    with torch.no_grad():
        dist.wG.mul_(-1.0)
    again = dist.component_cdf()
    assert again is not cdf and (again.double() - cdf_tables(dist.wG.detach())[0]).abs().max().item() <= 1e-7


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


def draw_call(mG, sG, cdf, labels, label0, u, eps, state, seed, z1, zbs, D1, out, B, M, K, D, T):
    from contextflow_amd.layers import _hip
    _hip.call("cf_gmm_draw", _hip.p(mG), _hip.p(sG), _hip.p(cdf), _hip.p(labels), label0, _hip.p(u), _hip.p(eps), _hip.p(state), seed,
              _hip.p(z1), zbs, D1, _hip.p(out), B, M, K, D, T, _hip.stream())
    torch.cuda.synchronize()


def shifted(t):
    """A copy of t that starts 4 bytes behind a 16-byte boundary."""
    s = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)[1:].view(t.shape)
    s.copy_(t)
    assert s.data_ptr() % 16 == 4
    return s


def framed(B, W, off=0):
    """(buffer full of sentinels, its (B, W) window `off` floats behind the aligned position)."""
    buf = torch.full((B * W + 2 * PAD + 1,), SENT, device=DEV)
    return buf, buf[PAD + off:PAD + off + B * W].view(B, W)


def frame_intact(buf, B, W, off=0):
    return bool(torch.all(buf[:PAD + off] == SENT) and torch.all(buf[PAD + off + B * W:] == SENT))


def close(out, ref):
    return ((out.cpu().double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item() if ref.numel() else 0.0


def pick_uniforms(c64, labels, g):
    """B uniforms whose component is unambiguous: the first K samples sit in the middle of component 0 .. K-1's interval of
    their class, the others are random, and whatever lies within 1e-4 of a boundary moves to the middle of its interval
    (the fp32 and the fp64 boundaries differ by 1e-7).  Returns (u fp32, k expected)."""
    B, K = labels.shape[0], c64.shape[1]
    if B == 0:
        return torch.empty(0), torch.empty(0, dtype=torch.long)
    lo = torch.cat([torch.zeros(c64.shape[0], 1, dtype=torch.float64), c64[:, :-1]], 1)[labels]      # (B, K) interval starts
    hi = c64[labels].clone()
    hi[:, -1] = 1.0
    mid = 0.5 * (lo + hi)
    u = torch.rand(B, generator=g).double()
    n = min(B, K)
    u[:n] = mid[torch.arange(n), torch.arange(n)]
    k = (u[:, None] >= hi).sum(1).clamp(max=K - 1)
    near = ((u[:, None] - hi[:, :-1]).abs() < 1e-4).any(1)
    u = torch.where(near, mid[torch.arange(B), k], u).float()
    k = (u.double()[:, None] >= hi).sum(1).clamp(max=K - 1)
    assert ((u.double()[:, None] - hi[:, :-1]).abs() >= 5e-5).all() and u.max().item() < 1.0
    return u, k


@pytest.mark.gpu
@pytest.mark.parametrize("D", [2048, 96, 7, 1])
def test_draw_kernel_with_explicit_noise(L, D):
    """cf_gmm_draw, u and eps given: (M, K) = (3, 5), D1 in {0, D, 3}, B in {1, 3, 1001, 0}, temperature in {1, 0.7, 0}, labels that
    hit class 0 and class M - 1 (per sample, and through label0 with labels == NULL), every component picked.  Upper half
    against mG + T softplus(sG) eps in fp64: 1e-6 of max(1, |out|); lower half bitwise z1, from a dense and from a
    batch-strided z1; sentinels on both sides of the output; every operand in turn 4 bytes off a 16-byte boundary gives the
    bits of the aligned run."""
    M, K = 3, 5
    g = torch.Generator().manual_seed(1000 + D)
    mG = (3.0 * torch.randn(M * K, D, generator=g)).to(DEV)
    sG = (8.0 * torch.rand(M * K, D, generator=g) - 4.0).to(DEV)           # softplus from 0.018 to 4.02
    wG = 2.0 * torch.rand(M, K, generator=g) - 1.0
    c64, c32 = cdf_tables(wG)
    cdf = c32.to(DEV)
    m64, sp64 = mG.cpu().double(), F.softplus(sG.cpu().double())
    worst, picked = 0.0, set()
    for B in (1, 3, 1001, 0):
        for label0 in ((0, M - 1) if B == 1 else (None,)):
            nb = max(B, 1)
            if label0 is None:
                lab = torch.randint(0, M, (nb,), generator=g)
                lab[0], lab[-1] = 0, M - 1
            else:
                lab = torch.full((nb,), label0, dtype=torch.long)
            lab = lab[:B]
            u, k = pick_uniforms(c64, lab, g)
            picked.update(k.tolist())
            if B == 1001:
                assert set(k.tolist()) == set(range(K)) and {0, M - 1} <= set(lab.tolist())
            eps = torch.randn(B, D, generator=g)
            rows = lab * K + k
            base, spread = m64[rows], sp64[rows] * eps.double()            # ref = base + T spread
            lab_d = None if label0 is not None else lab.to(DEV, torch.int32)
            u_d, eps_d = u.to(DEV), eps.to(DEV)
            for D1 in (0, D, 3):
                W = D1 + D
                z1 = torch.randn(B, D1, generator=g).to(DEV) if D1 else None
                for T in (1.0, 0.7, 0.0):
                    ref = base + T * spread
                    buf, out = framed(B, W)
                    draw_call(mG, sG, cdf, lab_d, label0 or 0, u_d, eps_d, None, 0, z1, D1, D1, out, B, M, K, D, T)
                    assert frame_intact(buf, B, W), (B, D1, T)
                    e = close(out[:, D1:], ref)
                    worst = max(worst, e)
                    assert e <= 1e-6, (B, D1, T, e)
                    if D1:
                        assert torch.equal(out[:, :D1], z1), (B, D1, T)
                    if T == 0.0 and B:
                        assert torch.equal(out[:, D1:], mG[rows.to(DEV)])          # fma(0, eps, mG)
                    if B == 0 or T != 0.7:
                        continue
                    # the kept half as a channel slice of a wider tensor: batch stride D1 + 8, 16 bytes into each row
                    if D1:
                        wide = torch.full((B, D1 + 8), -7.0, device=DEV)
                        zs = wide[:, 4:4 + D1]
                        zs.copy_(z1)
                        buf2, out2 = framed(B, W)
                        draw_call(mG, sG, cdf, lab_d, label0 or 0, u_d, eps_d, None, 0, zs, D1 + 8, D1, out2, B, M, K, D, T)
                        assert frame_intact(buf2, B, W) and torch.equal(out2, out), (B, D1, "strided z1")
                    # every operand in turn 4 bytes off a 16-byte boundary: the scalar form, the same bits
                    for which in ("mG", "sG", "eps", "z1", "out", "u", "cdf"):
                        if which == "z1" and not D1:
                            continue
                        a = dict(mG=mG, sG=sG, eps=eps_d, z1=z1, u=u_d, cdf=cdf)
                        if which != "out":
                            a[which] = shifted(a[which])
                        off = 1 if which == "out" else 0
                        buf2, out2 = framed(B, W, off)
                        assert out2.data_ptr() % 16 == 4 * off
                        draw_call(a["mG"], a["sG"], a["cdf"], lab_d, label0 or 0, a["u"], a["eps"], None, 0, a["z1"], D1, D1, out2,
                                  B, M, K, D, T)
                        assert frame_intact(buf2, B, W, off), (B, D1, which)
                        assert torch.equal(out2, out), (B, D1, which)
    assert picked == set(range(K))
    print("cf_gmm_draw D=%d: worst error %.2e of max(1, |out|) (bar 1e-06)" % (D, worst))


def philox_setup(M, K, D, seed):
    g = torch.Generator().manual_seed(seed)
    mG = (3.0 * torch.randn(M * K, D, generator=g)).to(DEV)
    sG = (2.0 * torch.rand(M * K, D, generator=g) - 1.0).to(DEV)
    wG = 2.0 * torch.rand(M, K, generator=g) - 1.0
    return mG, sG, wG, cdf_tables(wG)[1].to(DEV)


def philox_draw(mG, sG, cdf, lab, B, M, K, D, T, state, seed=0x1234ABCD5678, out=None):
    st = torch.tensor([state], device=DEV, dtype=torch.int64)
    if out is None:
        out = torch.empty(B, D, device=DEV)
    draw_call(mG, sG, cdf, lab, 0, None, None, st, seed, None, 0, 0, out, B, M, K, D, T)
    return out


def implied_components(x0, mG, lab, M, K):
    """k per row of a temperature-0 draw: the row must be bitwise exactly one of the K mean rows of its own class."""
    means = mG.view(M, K, -1)[lab.long()]                              # (B, K, D)
    hit = (x0[:, None, :] == means).all(-1)
    assert bool((hit.sum(1) == 1).all())
    return hit.float().argmax(1)


@pytest.mark.gpu
def test_philox_component_frequencies(L):
    """M = 3, K = 8, D = 4, 20 000 samples per class, temperature 0: every row is one of the mean rows of its own class and
    the component frequencies per class are within 5 sigma of softmax(wG[m]) (min p_k >= 0.019)."""
    M, K, D, per = 3, 8, 4, 20000
    B = M * per
    mG, sG, wG, cdf = philox_setup(M, K, D, 5)
    lab = (torch.arange(B) % M).to(DEV, torch.int32)
    x0 = philox_draw(mG, sG, cdf, lab, B, M, K, D, 0.0, state=77)
    k = implied_components(x0, mG, lab, M, K)
    p = torch.softmax(wG.double(), -1)
    assert p.min().item() >= 0.019
    for m in range(M):
        freq = torch.bincount(k[lab == m].cpu(), minlength=K).double() / per
        dev = ((freq - p[m]).abs() / (5.0 * torch.sqrt(p[m] * (1 - p[m]) / per))).max().item()
        print("class %d: component frequencies at most %.2f of the 5 sigma bar from softmax(wG)" % (m, dev))
        assert dev <= 1.0, (m, freq, p[m])


@pytest.mark.gpu
def test_philox_noise_moments_and_temperature(L):
    """B = 1024, D = 64 (65 536 normals), the same (seed, state) at T = 0, 0.5 and 1: the implied eps = (x_T1 - x_T0) / softplus(sG)
    has the moments and lag-1 correlations test_in_kernel_noise_statistics asks of the Augment noise, and the draw at 0.5
    lies halfway - the component and eps do not depend on the temperature."""
    M, K, D, B = 3, 8, 64, 1024
    mG, sG, wG, cdf = philox_setup(M, K, D, 6)
    lab = (torch.arange(B) % M).to(DEV, torch.int32)
    x0, xh, x1 = (philox_draw(mG, sG, cdf, lab, B, M, K, D, T, state=3) for T in (0.0, 0.5, 1.0))
    k = implied_components(x0, mG, lab, M, K)
    sp = F.softplus(sG.double()).view(M, K, D)[lab.long(), k.long()]
    eps = ((x1.double() - x0.double()) / sp).cpu()
    mom = [eps.mean().item(), eps.var().item(), (eps ** 3).mean().item(), (eps ** 4).mean().item()]
    cd = torch.corrcoef(torch.stack([eps[:, :-1].flatten(), eps[:, 1:].flatten()]))[0, 1].abs().item()
    cb = torch.corrcoef(torch.stack([eps[:-1].flatten(), eps[1:].flatten()]))[0, 1].abs().item()
    half = ((xh.double() - x0.double()) - 0.5 * (x1.double() - x0.double())).abs() / x1.double().abs().clamp_min(1.0)
    print("implied eps: mean %.3e var %.4f third %.3e fourth %.4f, lag-1 along d %.2e along b %.2e; T=0.5 off halfway by %.2e"
          % (*mom, cd, cb, half.max().item()))
    assert abs(mom[0]) < 2e-2 and abs(mom[1] - 1.0) < 3e-2 and abs(mom[2]) < 5e-2 and abs(mom[3] - 3.0) < 0.15
    assert cd < 1e-2 and cb < 1e-2
    assert half.max().item() <= 1e-6


@pytest.mark.gpu
def test_philox_repeatability(L):
    """Same (seed, state): the same bits; state + 1: other numbers; an output 4 bytes off a 16-byte boundary (the scalar
    form of the kernel): the same bits - with a ragged D too, where only the scalar form exists."""
    M, K, B = 3, 8, 257
    for D in (64, 7):
        mG, sG, wG, cdf = philox_setup(M, K, D, 7 + D)
        lab = (torch.arange(B) % M).to(DEV, torch.int32)
        a = philox_draw(mG, sG, cdf, lab, B, M, K, D, 0.7, state=11)
        b = philox_draw(mG, sG, cdf, lab, B, M, K, D, 0.7, state=11)
        c = philox_draw(mG, sG, cdf, lab, B, M, K, D, 0.7, state=12)
        buf, win = framed(B, D, 1)
        d = philox_draw(mG, sG, cdf, lab, B, M, K, D, 0.7, state=11, out=win)
        assert torch.equal(a, b) and not torch.equal(a, c)
        assert frame_intact(buf, B, D, 1) and torch.equal(a, d)
        if D % 4 == 0:      # a row length that is no multiple of 4 sees the same noise in its first elements
            mG7, sG7 = mG[:, :7].contiguous(), sG[:, :7].contiguous()
            # (another D moves the counter base of every sample but the first: compare sample 0)
            e = philox_draw(mG7, sG7, cdf, lab, B, M, K, 7, 0.7, state=11)
            assert torch.equal(e[0], a[0, :7])


@pytest.mark.gpu
def test_distribution_sample_with_labels(L):
    """GaussianMixtureDistribution.sample(n, labels=, temperature=): M = 4, size (8, 4, 4), n = 2048, labels = arange(n) % 4.  The
    returned log-density is log_prob of the returned x (1e-6, the `close` of test_sample_shapes_and_prior_consistency); the samples
    of class c score highest under class-mixture c; torch.manual_seed reproduces the draw bitwise and another seed does not;
    bad labels raise ValueError."""
    M, size, n = 4, (8, 4, 4), 2048
    torch.manual_seed(4)
    dist = L.GaussianMixtureDistribution(size=size, mixtures=M, components=8).to(DEV)
    labels = torch.arange(n) % M
    torch.manual_seed(21)
    x, lp = dist.sample(n, labels=labels)
    torch.manual_seed(21)
    x2, none = dist.sample(n, need_log_prob=False, labels=labels.to(DEV))
    torch.manual_seed(22)
    x3, _ = dist.sample(n, labels=labels)
    assert tuple(x.shape) == (n,) + size and tuple(lp.shape) == (n, M) and none is None
    assert torch.equal(x, x2) and not torch.equal(x, x3)
    ref = dist.log_prob(x)
    e = ((lp - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
    assert e <= 1e-6
    for c in range(M):
        assert int(lp[(labels == c).to(DEV)].mean(0).argmax()) == c
    # temperature alone: class-mixture 1, and temperature 0 collapses every sample onto a component mean of it
    x0, _ = dist.sample(64, temperature=0.0)
    means = dist.mG.detach()[1].reshape(8, -1)
    assert bool(((x0.reshape(64, 1, -1) == means[None]).all(-1).sum(1) == 1).all())
    # a tuple of class indices is a sequence like any other (never taken for the prepared form the flow hands down), here and in
    # SplitPrior.reverse; a 0-dim device tensor is that class for every sample
    torch.manual_seed(21)
    x4, _ = dist.sample(n, need_log_prob=False, labels=tuple(labels.tolist()))
    assert torch.equal(x, x4)
    a2, _ = dist.sample(2, need_log_prob=False, labels=(0, 3), temperature=0.0)
    for row, c in zip(a2, (0, 3)):
        assert bool((row.reshape(1, -1) == dist.mG.detach()[c].reshape(8, -1)).all(-1).any())
    split = L.SplitPrior(dist)
    z = torch.randn(4, *size, device=DEV)
    back = split.reverse(z, labels=(3, 2, 1, 0), temperature=0.0)
    assert tuple(back.shape) == (4, 2 * size[0]) + size[1:] and torch.equal(back[:, :size[0]], z)
    for row, c in zip(back[:, size[0]:], (3, 2, 1, 0)):
        assert bool((row.reshape(1, -1) == dist.mG.detach()[c].reshape(8, -1)).all(-1).any())
    x5, _ = dist.sample(16, need_log_prob=False, labels=torch.tensor(2, device=DEV), temperature=0.0)
    assert bool(((x5.reshape(16, 1, -1) == dist.mG.detach()[2].reshape(1, 8, -1)).all(-1).sum(1) == 1).all())
    with pytest.raises(ValueError, match="outside"):
        dist.sample(n, labels=4)
    with pytest.raises(ValueError, match="shape"):
        dist.sample(3, labels=[0, 1])
    with pytest.raises(ValueError, match="shape"):
        dist.sample(3, labels=(0, 1))
    with pytest.raises(ValueError, match="outside"):
        dist.sample(2, labels=(0, 4))
    with pytest.raises(ValueError, match="labels"):
        dist.sample(2, labels=(None, 99))
    with pytest.raises(ValueError, match="integer"):
        dist.sample(2, labels=(0.0, 1.0))
    flow = L.FlowSequential(L.StandardNormal(size)).to(DEV)
    with pytest.raises(ValueError):
        flow.sample(3, labels=0)


@functools.lru_cache(maxsize=None)
def fixture_model(name):
    from tests.gpu_util import build_model
    ops, _, M, params, _ = load_e2e(name)
    return ops, params, M, build_model(name, params)


def mixture_levels(L, model):
    """The mixtures a sample passes, in forward order: every SplitPrior's, then the prior."""
    return [m.dist for m in model.sequence_modules if isinstance(m, L.SplitPrior)] + [model.dist]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cifar10", "mnist"])
def test_labels_reach_every_level(L, name):
    """One component per class carries all the weight in the prior and in every SplitPrior (wG = +-60: the cdf is exactly 0 / 1
    in fp32), a different one per class and level.  sample(10, labels=arange(10), temperature=0) is then decode(latents, clamp=True)
    of the latents made of those components' mean rows, bit for bit: the label of every sample arrived at every level."""
    from tests.gpu_util import build_model
    ops, _, M, params, _ = load_e2e(name)
    model = build_model(name, params)
    levels = mixture_levels(L, model)
    assert len(levels) == {"cifar10": 3, "mnist": 1}[name] and M == 10          # (the mnist flow has no SplitPrior: its prior alone)
    latents = []
    c = torch.arange(M)
    with torch.no_grad():
        for lv, dist in enumerate(levels):
            j = (3 * c + lv + 1) % dist.K
            dist.wG.fill_(-60.0)
            dist.wG[c, j] = 60.0
            cdf = dist.component_cdf()
            assert bool(((cdf == 0) | (cdf == 1)).all())
            latents.append(dist.mG.detach()[c, j].clone())
    got = model.sample(M, labels=c, temperature=0.0)
    want = model.decode(latents, clamp=True)
    assert tuple(got.shape) == (M,) + tuple(fo.CONFIGS[name][0])
    assert torch.equal(got, want)
    other = model.sample(M, labels=(c + 1) % M, temperature=0.0)
    assert not torch.equal(got, other) and torch.equal(other[:-1], got[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cifar10", "mnist"])
def test_flow_sample_with_labels_and_temperature(L, name):
    """sample(261, labels=, temperature=0.7) with the fixture weights: integer valued pixels inside [0, 255], repeatable under a
    seed, other pixels under another seed; a class outside [0, M) raises ValueError."""
    ops, params, M, model = fixture_model(name)
    B = 261
    labels = torch.arange(B) % M
    torch.manual_seed(3)
    a = model.sample(B, labels=labels, temperature=0.7)
    torch.manual_seed(3)
    b = model.sample(B, labels=labels.to(DEV), temperature=0.7)
    torch.manual_seed(4)
    c = model.sample(B, labels=labels, temperature=0.7)
    assert tuple(a.shape) == (B,) + tuple(fo.CONFIGS[name][0]) and a.dtype == torch.float32
    assert torch.isfinite(a).all() and torch.equal(a, a.floor())
    assert a.min().item() >= 0 and a.max().item() <= 255
    assert torch.equal(a, b) and not torch.equal(a, c)
    with pytest.raises(ValueError):
        model.sample(B, labels=M)


def traced(ops, params, x, u, eps, dtype):
    """Oracle forward with a trace in `dtype` -> (z, halves, inputs) (oracle.flow_oracle.inverse_problem)."""
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params.items()}
    tr = []
    x = x.to(dtype)
    fo.flow_forward(ops, p, x, u.to(dtype), [e.to(dtype) for e in eps], trace=tr)
    return fo.inverse_problem(ops, x, tr)


ENC_B = 37


@functools.lru_cache(maxsize=None)
def encode_problem(name):
    """37 random uint8 images, dequantisation noise in [1/64, 63/64], Augment noise; the fp64 oracle trace and the fp32 one."""
    ops, _, _, params, _ = load_e2e(name)
    C, H, W = fo.CONFIGS[name][0]
    g = torch.Generator().manual_seed(37 + C)
    x = torch.randint(0, 256, (ENC_B, C, H, W), generator=g).float()
    u = 1.0 / 64 + (1.0 - 2.0 / 64) * torch.rand(ENC_B, C, H, W, generator=g)
    eps = [torch.randn(ENC_B, 1, H, W, generator=g)]
    z, halves, _ = traced(ops, params, x, u, eps, torch.float64)
    z32, halves32, _ = traced(ops, params, x, u, eps, torch.float32)
    return x, u, eps, halves + [z], halves32 + [z32]


def err_of(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return (got - ref).abs().max().item() / max(1.0, ref.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cifar10", "mnist"])
def test_encode_against_forward_and_the_fp64_trace(L, name):
    """encode(x) with injected noise, B = 37, fused and layer by layer: logp and z are forward's bit for bit, one latent per
    SplitPrior plus z, each a fresh contiguous tensor, every one held against the fp64 oracle trace.  The bar is 1e-5 of the
    tensor's scale - what tests/test_sampling.py holds these tensors to in the other direction - where the reference's own
    arithmetic (the fp32 oracle forward on the same inputs, printed next to each figure) sits at least 3x under it, and 10x
    that floor otherwise.  On these inputs (uniformly random pixels, harsher than the fixtures' images) it does for neither
    fixture - fp32 oracle forward, worst latent: cifar10 1.56e-5 of scale, mnist 6.05e-6 - so the bars are 1.56e-4 for
    cifar10 and 6.05e-5 for mnist."""
    from tests.gpu_util import set_noise
    ops, params, M, model = fixture_model(name)
    x, u, eps, want, floor32 = encode_problem(name)
    n_split = sum(isinstance(m, L.SplitPrior) for m in model.sequence_modules)
    floor = max(err_of(r32, ref) for r32, ref in zip(floor32, want))
    bar = ACT_TOL if 3.0 * floor <= ACT_TOL else 10.0 * floor
    set_noise(model, u, eps)
    try:
        for fused in (True, False):
            model.fused = fused
            with torch.no_grad():
                z, logp = model(x.to(DEV))
            latents, logp_e = model.encode(x.to(DEV))
            assert torch.equal(logp_e, logp) and torch.equal(latents[-1], z)
            assert len(latents) == n_split + 1 == len(want)
            for i, (got, ref, r32) in enumerate(zip(latents, want, floor32)):
                assert got.is_contiguous() and got.dtype == torch.float32 and got._base is None
                e = err_of(got, ref)
                print("%s encode %s latent %d %s: %.2e of scale (fp32 oracle forward %.2e; bar %.2e)"
                      % (name, "fused" if fused else "layers", i, tuple(got.shape), e, err_of(r32, ref), bar))
                assert e <= bar, (fused, i, e)
    finally:
        model.fused = True
        set_noise(model, None, [])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cifar10", "mnist"])
def test_decode_of_encode_returns_every_pixel(L, name):
    """decode(encode(x)[0]) gives back every pixel of every one of 37 random uint8 images (dequantisation noise in [1/64, 63/64], as
    test_exact_pixel_cycle_at_a_ragged_batch), is bitwise `inverse(z)` with the same halves injected through set_split_draws,
    and clamp=True changes nothing on pixels that are inside the range; a missing latent or a half with the wrong channel
    count raises ValueError."""
    from tests.gpu_util import set_noise, set_split_draws
    ops, params, M, model = fixture_model(name)
    x, u, eps, _, _ = encode_problem(name)
    set_noise(model, u, eps)
    try:
        latents, _ = model.encode(x.to(DEV))
    finally:
        set_noise(model, None, [])
    back = model.decode(latents)
    wrong = back.cpu() != x
    print("%s decode(encode(x)): %d of %d pixels wrong" % (name, int(wrong.sum()), wrong.numel()))
    assert tuple(back.shape) == tuple(x.shape) and not wrong.any()
    with set_split_draws(model, latents[:-1]):
        plain = model.inverse(latents[-1])
    assert torch.equal(back, plain)
    assert torch.equal(model.decode(latents, clamp=True), back)
    with pytest.raises(ValueError):
        model.decode(latents[1:])
    with pytest.raises(ValueError):
        model.decode(latents + [latents[-1]])
    for i in range(len(latents)):                    # every half, and z, with a channel missing
        bad = list(latents)
        bad[i] = bad[i][:, :-1].contiguous()
        with pytest.raises(ValueError):
            model.decode(bad)
    for split in (m for m in model.sequence_modules if isinstance(m, L.SplitPrior)):
        with pytest.raises(ValueError):
            split.reverse(latents[0], latent=latents[0][:, :1])
