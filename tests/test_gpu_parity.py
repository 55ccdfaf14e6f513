"""GPU parity tests (run with -m gpu on the MI355X box).  Every test goes through the C ABI
(libcontextflow_hip.so via contextflow_amd.layers) and is checked against the oracle and/or the
committed golden vectors produced by the reference.  Tolerances: bits/dim 1e-5 (BASELINE.json),
activations 1e-5 relative to the tensor's scale."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flow_oracle as fo                     # noqa: E402
from tests.helpers import load_e2e, pre_init_params, e2e_inputs, unit, bpd, stress_tolerance, gmm_resp_closed_form   # noqa: E402

BPD_TOL = 1e-5
DEV = "cuda:0"


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


# ------------------------------------------------------------------------------------------ unit layers
@pytest.mark.parametrize("tag", ["coupling_3x3", "coupling_3x1", "coupling_c16"])
def test_coupling_generic(L, tag):
    t, sd = unit(tag)
    C = t["x"].shape[1]
    m = L.Coupling(C, kernel_size=tuple(int(v) for v in t["krn"]), padding=tuple(int(v) for v in t["pad"]))
    m.load_state_dict(sd)
    m = m.to(DEV)
    x = t["x"].to(DEV)
    close(m.net(x[:, : C // 2]), t["h"])
    z, ldj = m(x)
    close(z, t["z"]); close(ldj, t["ldj"])
    close(m.reverse(t["z"].to(DEV)), t["xrec"])
    close(m.reverse(z), t["x"])


@pytest.mark.parametrize("tag,size", [("conv1x1_c26", (26, 8, 1)), ("conv1x1_c64", (64, 4, 4))])
def test_conv1x1(L, tag, size):
    t, sd = unit(tag)
    m = L.Conv1x1(size)
    m.load_state_dict(sd)
    m = m.to(DEV)
    z, ldj = m(t["x"].to(DEV))
    close(z, t["z"])
    close(ldj, t["ldj"].expand_as(ldj), tol=1e-5)      # the reference LU is fp32, ours fp64
    close(m.reverse(t["z"].to(DEV)), t["xrec"], tol=1e-4)
    close(m.reverse(z), t["x"], tol=1e-4)


def test_actnorm_init_and_apply(L):
    t, sd = unit("actnorm")
    m = L.ActNorm((7, 3, 4)).to(DEV)
    z, ldj = m(t["x"].to(DEV))                       # first call: data-dependent init
    close(m.NN_t, sd["NN_t"], tol=1e-6); close(m.NN_logs, sd["NN_logs"], tol=1e-6)
    assert int(m.initialized.item()) == 1
    close(z, t["z"]); close(ldj, t["ldj"])
    z2, ldj2 = m(t["x2"].to(DEV))
    close(z2, t["z2"]); close(ldj2, t["ldj2"])
    close(m.reverse(t["z2"].to(DEV)), t["x2rec"])


def test_actnorm_sharded_init_equals_whole_batch(L):
    """cf_actnorm_sums + cf_actnorm_from_sums (the data-parallel init): sums of two ragged shards added
    together give the parameters of the whole-batch init, and the sharded_init code path of the layer (world size 1)
    reproduces the reference's post-init parameters."""
    from contextflow_amd.dist import sharded_actnorm_init
    from contextflow_amd.layers import _hip
    t, sd = unit("actnorm")
    x = t["x"].to(DEV)
    B, C = x.shape[0], x.shape[1]
    HW = x.shape[2] * x.shape[3]
    lib = _hip.lib()
    tot = torch.zeros(2 * C, device=DEV, dtype=torch.float64)
    for lo, hi in ((0, 3), (3, B)):
        xs = x[lo:hi].contiguous()
        sums = torch.empty(2 * C, device=DEV, dtype=torch.float64)
        ws = torch.empty(lib.cf_actnorm_stats_ws_bytes(C), device=DEV, dtype=torch.uint8)
        _hip.call("cf_actnorm_sums", _hip.p(xs), _hip.p(sums), _hip.p(ws), hi - lo, C, HW, C * HW, _hip.stream())
        tot += sums
    tt, logs = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    cnt = torch.tensor([float(B * HW)], device=DEV, dtype=torch.float64)
    _hip.call("cf_actnorm_from_sums", _hip.p(tot), _hip.p(cnt), 0.0, _hip.p(tt), _hip.p(logs), C, _hip.stream())
    close(tt, sd["NN_t"], 1e-6); close(logs, sd["NN_logs"], 1e-6)
    m = L.ActNorm((C, x.shape[2], x.shape[3])).to(DEV)
    with sharded_actnorm_init():
        z, _ = m(x)
    assert m.is_initialized()
    close(m.NN_t, sd["NN_t"], 1e-6); close(m.NN_logs, sd["NN_logs"], 1e-6)
    close(z, t["z"])


def test_squeeze(L):
    t, _ = unit("squeeze22")
    s = L.Squeeze((2, 2))
    z, ldj = s(t["x"].to(DEV))
    assert torch.equal(z.cpu(), t["z"]) and float(ldj.abs().sum()) == 0.0
    assert torch.equal(s.reverse(z).cpu(), t["xrec"])
    t, _ = unit("squeeze21")
    assert torch.equal(L.Squeeze((2, 1))(t["x"].to(DEV))[0].cpu(), t["z"])


def test_gmm_and_splitprior(L):
    t, sd = unit("gmm")
    m = L.GaussianMixtureDistribution(size=(5, 3, 2), mixtures=3, components=8)
    m.load_state_dict(sd)
    close(m.to(DEV).log_prob(t["x"].to(DEV)), t["logp"])
    t, sd = unit("split")
    sp = L.SplitPrior(L.GaussianMixtureDistribution(size=(5, 3, 2), mixtures=2, components=8))
    sp.load_state_dict(sd)
    z, ldj = sp.to(DEV)(t["x"].to(DEV))
    assert torch.equal(z.cpu(), t["z"])
    close(ldj, t["ldj"])


def test_gmm_split_d_matches_single_pass(L):
    """The D-split (workspace) form and the single-pass form are the same sum."""
    from contextflow_amd.layers.distributions.gaussian import gmm_prepare, gmm_logprob
    from contextflow_amd.layers import _hip
    g = torch.Generator().manual_seed(3)
    M, K, D, B = 10, 8, 2048, 300
    mG, sG, wG = torch.randn(M, K, D, generator=g), 1 + 0.2 * torch.randn(M, K, D, generator=g), torch.randn(M, K, generator=g)
    x = torch.randn(B, D, generator=g)
    prep = gmm_prepare(mG.to(DEV), sG.to(DEV), wG.to(DEV))
    a, nm, cst = prep[:3]
    out1 = torch.empty(B, M, device=DEV)
    xd = x.to(DEV)
    _hip.call("cf_gmm_logprob", _hip.p(xd), _hip.p(a), _hip.p(nm), _hip.p(cst), _hip.p(out1), _hip.p(None), B, M, K, D, D, 0, _hip.stream())
    out2 = gmm_logprob(xd, prep)
    assert _hip.lib().cf_gmm_ws_bytes(B, M, K, D) > 0
    close(out1, fo.gmm_logprob(x, mG, sG, wG), tol=2e-6)
    close(out2, out1, tol=1e-6)


@pytest.mark.parametrize("B,with_ldM", [(1, False), (70, True), (256, False), (1000, True)])
def test_gmm_levels_entry_equals_the_chain_of_calls(L, B, with_ldM):
    """cf_gmm_logprob_levels (all mixtures of a flow in one launch pair, small batches) = the chain of accumulating
    cf_gmm_logprob calls + cf_logdet_combine, bit for bit; levels are channel slices of wider tensors as in the flow."""
    from contextflow_amd.layers.distributions.gaussian import gmm_prepare, gmm_logprob, gmm_levels_ok, gmm_logprob_levels
    from contextflow_amd.layers import _hip
    g = torch.Generator().manual_seed(11 + B)
    M, K = 10, 8
    levels, ref = [], []
    for D, wide in ((1536, 3072), (768, 1536), (768, 768)):
        mG, sG, wG = torch.randn(M, K, D, generator=g), 1 + 0.2 * torch.randn(M, K, D, generator=g), torch.randn(M, K, generator=g)
        xw = torch.randn(B, wide, generator=g).to(DEV)
        x = xw[:, wide - D:]
        levels.append((x, gmm_prepare(mG.to(DEV), sG.to(DEV), wG.to(DEV))))
        ref.append(fo.gmm_logprob(x.cpu(), mG, sG, wG))
    ld1 = torch.randn(B, generator=g).to(DEV)
    ldM0 = torch.randn(B, M, generator=g).to(DEV) if with_ldM else None
    assert gmm_levels_ok(levels)
    got = gmm_logprob_levels(levels, ldM0, ld1)
    ldM = ldM0.clone() if with_ldM else torch.empty(B, M, device=DEV)
    for i, (x, prep) in enumerate(levels):
        gmm_logprob(x, prep, out=ldM, accumulate=with_ldM or i > 0)
    want = torch.empty(B, M, device=DEV)
    _hip.call("cf_logdet_combine", _hip.p(ldM), _hip.p(ld1), _hip.p(want), B, M, _hip.stream())
    assert torch.equal(got, want)
    _gmm_bits("levels", (B, with_ldM), [got])
    tot = sum(ref) + ld1.cpu()[:, None] + (ldM0.cpu() if with_ldM else 0)
    close(got, tot, tol=3e-6)
    assert not gmm_levels_ok([(levels[0][0][:, 1:], levels[0][1])])          # misaligned / wrong width: refused, not copied


@pytest.mark.parametrize("B,contexts", [(5000, [15, 5]), (700, [3, 2]), (129, [1, 1])])
def test_keyed_mixture_kernel_against_the_formula_and_the_per_sample_kernel(L, B, contexts):
    """Context-shifted mixtures with embedding-lookup shifts at batches with many samples per context value run the
    register-tiled kernel over samples bucketed by key (cf_gmm_logprob_keyed): against gaussian.py:142-158 in fp64 and
    against the per-sample table kernel it replaces there; empty buckets, ragged tiles, one bucket only."""
    from contextflow_amd.layers.distributions import gaussian as G
    from contextflow_amd.layers.context import CatEmbeddings, EyeSampling
    torch.manual_seed(B)
    D, H, W, M, K = 6, 8, 8, 10, 8
    half = M * K * D
    cn = torch.nn.Sequential(CatEmbeddings(contexts, 2 * half // len(contexts), stack=False, init="zeros"), EyeSampling())
    cn.C = 2 * half
    dist = G.GaussianMixtureDistribution((D, H, W), mixtures=M, components=K, contextflow=True, context_net=cn)
    with torch.no_grad():
        dist.mG.mul_(0.5); dist.sG.copy_(0.5 * torch.randn_like(dist.sG) + 0.5)
        for e in dist.context_net[0]._embeddings:
            e.weight.copy_(0.3 * torch.randn_like(e.weight))
    dist = dist.to(DEV)
    x = torch.randn(B, D, H, W, device=DEV)
    context = torch.stack([torch.randint(0, k, (B,)) for k in contexts], 1)
    if contexts[0] > 3:
        context[context[:, 0] == 2, 0] = 3                                   # an empty bucket
    context = context.to(DEV)
    with torch.no_grad():
        got = dist.log_prob(x, context)
        assert G._bucket_cache[0] is not None and G._bucket_cache[0][0] is context, "the keyed path did not run"
        keep, G.KEYED_MIN_PER_KEY = G.KEYED_MIN_PER_KEY, 1 << 30
        try:
            per_sample = dist.log_prob(x, context)
        finally:
            G.KEYED_MIN_PER_KEY = keep
        c, _ = dist.context_net(context)
    c = c.double().cpu().view(B, 2, M, K, D, 1, 1)
    mu = dist.mG.double().cpu().unsqueeze(0) + c[:, 0]
    sig = torch.nn.functional.softplus(dist.sG.double().cpu().unsqueeze(0) + c[:, 1])
    lp = (-0.5 * ((x.double().cpu().view(B, 1, 1, D, H, W) - mu) / sig) ** 2 - torch.log(sig) - 0.5 * math.log(2 * math.pi)).flatten(3).sum(-1)
    ref = torch.logsumexp(lp + torch.log_softmax(dist.wG.double().cpu(), -1), -1)
    scale = ref.abs().max().item()
    assert (got.cpu().double() - ref).abs().max().item() < 2e-6 * scale
    assert (got - per_sample).abs().max().item() < 2e-6 * scale
    # a new context tensor (other values, possibly the recycled storage) is bucketed afresh
    context2 = context.flip(0).clone()
    with torch.no_grad():
        got2 = dist.log_prob(x.flip(0).contiguous(), context2)
    assert torch.equal(got2, got.flip(0)) or (got2 - got.flip(0)).abs().max().item() < 2e-6 * scale


# ---- bits of the mixture entry points ---------------------------------------------------------------------------------------
# sha256 over the output bytes, recorded on an MI355X from the library as it was BEFORE cf_gmm.hip got its one launch plan and its
# shared finishing pieces (commit bbf7a47; two processes, equal digests: profiles/gmm_plan_parity.txt).  The inputs come from
# seeded CPU generators and every sum in these kernels has a fixed order, so the digests hold from run to run.
GMM_SHA = {
    "logprob": {
        (10, 8, 768, 70, 1536): "77934101c51abbd204c34251d8e4c4aaf6664a40fb134fba2363429dce2f24f5",
        (10, 8, 1536, 1, 1536): "7c88875179c50c45f862861794034169f077607367a29de9388f7476e2925032",
        (10, 8, 100, 300, 100): "bded5adbbfe0feb3d34194c64a15c43caee903c03aaad241ed076da0c7fa8506",
        (10, 8, 99, 131, 99): "15817742310d377904170dc53681d87160d84c797a53de24a1cae8c380eb38d2",
        (10, 8, 48, 257, 48): "0db8de9c4d6d5bd4099a542431dffd6d3427ec0c3df0b651e6929120cab6dbbb",
        (2, 8, 768, 70, 768): "99c08f5f577aeb724657e02eb8491b8677e6b1d3c52eb5101b226eb8f078f7f3",
        (1, 5, 64, 5, 64): "5c6f315e706b575a1e3bed0db94aae60c450c85fa8ccc8368a5ba277a027ba78",
        (5, 8, 768, 70, 768): "c836f5f4af851522593b785d7d513e90b4c9a1340e63b27f6789326552f96180",
        (33, 8, 256, 40, 256): "7e63de3ca7f5d9ad597469255e9d7f41d256fc686db257276587b6e4bd68507d",
    },
    "accumulate": {
        (10, 8, 768, 70, 1536): "995cea89ed0ef89e0a45bfed5275229460d0594d363b5650e1dd44cf730fa34f",
    },
    "single": {
        (10, 8, 768, 70, 1536): "d71f533187992e98fe9f991d8ee0b30596382050246b45c5e67c6642d9779b1b",
    },
    "resp": {
        (10, 8, 768, 70, 1536): "4f65b8d911cfe20700270b102ca8397a5359ae8d7153b81f98fd4c72f78926e6",
        (10, 8, 1536, 1, 1536): "81fc844ac62b1e2b2cd3b39b1d277971dde074b333a5f3084f143bfa7b99609d",
        (10, 8, 100, 300, 100): "b2fc3621175050f00fc329949f548ce8215838b9213c0a45014d3eed2d3a62d9",
        (10, 8, 99, 131, 99): "3c52e911c188bc996680dc9a587912461be7226f8ac1159f6fc8e3f0c2203099",
        (10, 8, 48, 257, 48): "12e17e28685b1a4575644afb3e10122904fb675ca624e48e70c0f16cb9e7b755",
        (2, 8, 768, 70, 768): "6e3ed5d687c03f941370279b54c05b3df8d072250ab4238b290d599a2137979d",
        (1, 5, 64, 5, 64): "f7b6a358e9b5873d952f4840603ea63ac7c11f8890261c54690d7d350e5bf173",
        (5, 8, 768, 70, 768): "c04acf449d22fa0bc1dd2fcc03f871cb4302d8b18f9fbb303a7f68957787fa85",
        (33, 8, 256, 40, 256): "15eac2d5e39e0606cb6a4b6b7410c5b78286ce09fbc4ad361c584bbd26db54c9",
    },
    "levels": {
        (1, False): "8ceb26d274eb67637034070f6bd3d754c5fbfc091f0286a7ded9e158188c2c6b",
        (70, True): "951d56c77db4c33db934c7e90a3a102d930314698671c0da44aa62c65aad1052",
        (256, False): "d44d040acb7c962025c6649377a70497980e3dd205ca37f246aafdaa4ae407f9",
        (1000, True): "81b1c9a16c112388025ef75f812c748929fe2997fbf5cb23fbf38c293fe2cfce",
    },
    "keyed": {
        (300, 0): "e9e9d963b011d3b1ed8da6cac7dbf19a5de3b76113c819dbfeceb23c5aeb0353",
        (300, 1): "54977e558b5d52a5ed19e5373339c5192c6d152739ce5c65f4328b673e6af415",
    },
}


def _gmm_bits(test, key, tensors):
    import hashlib
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    print("GMM_SHA %s %r %s" % (test, key, h.hexdigest()))
    assert GMM_SHA[test].get(key) == h.hexdigest(), (test, key, h.hexdigest())


# (M, K, D, B, row stride of x, d-slices launched): the smallest shapes that reach each branch of gmm_plan / gmm_launch and each
# finishing kernel.  768 columns off a channel slice in 12 slices (a tree group of 8 + a tail of 4); 24 slices for one sample;
# a ragged last chunk (second slice 36 wide); D % 4 != 0 (scalar loads); D < 64: no split, the in-body epilogue with a ragged
# sample tile; M K = 16 (one component per thread); M = 1 with 16 % K != 0; M K = 40: a ragged component block, 240-thread finish
# blocks; M K = 264 > 256: four component blocks, the last ragged, and the one-thread-per-(b, m) finishing kernels.
GMM_CASES = [(10, 8, 768, 70, 1536, 12), (10, 8, 1536, 1, 1536, 24), (10, 8, 100, 300, 100, 2), (10, 8, 99, 131, 99, 2),
             (10, 8, 48, 257, 48, 1), (2, 8, 768, 70, 768, 12), (1, 5, 64, 5, 64, 2), (5, 8, 768, 70, 768, 12),
             (33, 8, 256, 40, 256, 8)]
GMM_IDS = ["-".join(map(str, c[:5])) for c in GMM_CASES]
_gmm_case_cache, _gmm_case_cpu, _gmm_resp_cache = {}, {}, {}


def _gmm_case(case):
    """Seeded CPU inputs of a GMM_CASES entry, its prepared tables on the device and the oracle's log-probabilities (computed
    once, shared by the tests below, never written to)."""
    from contextflow_amd.layers.distributions.gaussian import gmm_prepare
    if case not in _gmm_case_cache:
        M, K, D, B, stride, _ = case
        g = torch.Generator().manual_seed(1000 * D + B)
        mG, sG, wG = torch.randn(M, K, D, generator=g), 1 + 0.2 * torch.randn(M, K, D, generator=g), torch.randn(M, K, generator=g)
        xw = torch.randn(B, stride, generator=g)
        out0, gup = torch.randn(B, M, generator=g), torch.randn(B, M, generator=g)
        x = xw.to(DEV)[:, stride - D:]                                        # a channel slice where stride > D
        ref = fo.gmm_logprob(xw[:, stride - D:], mG, sG, wG)
        _gmm_case_cache[case] = (x, gmm_prepare(mG.to(DEV), sG.to(DEV), wG.to(DEV)), out0, gup, ref)
        _gmm_case_cpu[case] = (xw[:, stride - D:], mG, sG, wG)
    return _gmm_case_cache[case]


def _gmm_case_resp(case):
    """cf_gmm_resp's result for the case by the closed form (tests/helpers.py) in fp64, and the relative error the same form makes
    in fp32 on these inputs - computed once."""
    if case not in _gmm_resp_cache:
        _, _, _, gup, _ = _gmm_case(case)
        xs, mG, sG, wG = _gmm_case_cpu[case]
        r64 = gmm_resp_closed_form(xs.double(), mG.double(), sG.double(), wG.double(), gup.double())
        r32 = gmm_resp_closed_form(xs, mG, sG, wG, gup)
        scale = max(r64.abs().max().item(), 1e-3)
        _gmm_resp_cache[case] = (r64, scale, (r32.double() - r64).abs().max().item() / scale)
    return _gmm_resp_cache[case]


def _gmm_slices_launched(case):
    """The slice count of the case as the library reports it: cf_gmm_levels_ws_bytes of the one level is the launched count x B M K
    floats (the plan of the cf_gmm_logprob call, literally); cf_gmm_ws_bytes and cf_gmm_resp_ws_bytes cover it (they report the
    count before the slices were rounded to 32 columns) and the former is 0 without a split."""
    from contextflow_amd.layers import _hip
    M, K, D, B, _, ns = case
    lib, per = _hip.lib(), B * M * K * 4
    assert lib.cf_gmm_levels_ws_bytes(1, (ctypes.c_int * 1)(D), B, M, K) == ns * per, case
    nb, nr = lib.cf_gmm_ws_bytes(B, M, K, D), lib.cf_gmm_resp_ws_bytes(B, M, K, D)
    assert (nb == 0 if ns == 1 else nb >= ns * per) and nr >= ns * per and nr == max(nb, per), case
    return nb, nr


@pytest.mark.parametrize("case", GMM_CASES, ids=GMM_IDS)
def test_gmm_logprob_bits_and_oracle(L, case):
    """cf_gmm_logprob at every branch of its plan: the recorded bits, and the oracle at 2e-6 (a wrong recording cannot hide a wrong
    kernel).  The first case also accumulating onto a seeded out and, without a workspace, through the single-pass epilogue."""
    from contextflow_amd.layers import _hip
    M, K, D, B, stride, ns = case
    x, (a, nm, cst, _, _, _), out0, _, ref = _gmm_case(case)
    nbytes, _ = _gmm_slices_launched(case)
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8) if nbytes else None

    def run(out, ws, accumulate):
        _hip.call("cf_gmm_logprob", _hip.p(x), _hip.p(a), _hip.p(nm), _hip.p(cst), _hip.p(out), _hip.p(ws), B, M, K, D, stride,
                  accumulate, _hip.stream())
        return out
    out = run(torch.empty(B, M, device=DEV), ws, 0)
    _gmm_bits("logprob", case[:5], [out])
    close(out, ref, tol=2e-6)
    if case == GMM_CASES[0]:
        acc = run(out0.to(DEV), ws, 1)
        _gmm_bits("accumulate", case[:5], [acc])
        close(acc, out0 + ref, tol=2e-6)
        single = run(torch.empty(B, M, device=DEV), None, 0)
        _gmm_bits("single", case[:5], [single])
        close(single, ref, tol=2e-6)


@pytest.mark.parametrize("case", GMM_CASES, ids=GMM_IDS)
def test_gmm_resp_bits(L, case):
    """cf_gmm_resp (responsibilities x upstream gradient) on the same shapes: the recorded bits; the responsibilities of a mixture
    sum to one (K roundings of a value <= 1: 1e-5 of the gradient's scale); r against softmax_k(log-joint + log-weight) * g in fp64,
    below max(1e-4, 3 x the error of the same form in fp32)."""
    from contextflow_amd.layers import _hip
    M, K, D, B, stride, ns = case
    x, (a, nm, cst, _, _, _), _, gup, _ = _gmm_case(case)
    _, nbytes = _gmm_slices_launched(case)
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    g = gup.to(DEV)
    r = torch.empty(B, M * K, device=DEV)
    _hip.call("cf_gmm_resp", _hip.p(x), _hip.p(a), _hip.p(nm), _hip.p(cst), _hip.p(g), _hip.p(r), _hip.p(ws), B, M, K, D, stride,
              _hip.stream())
    _gmm_bits("resp", case[:5], [r])
    close(r.view(B, M, K).sum(-1), gup, tol=1e-5)
    # ... and the values themselves, under the rule of tests/test_gmm_backward.py (recorded bits say "unchanged", not "right")
    r64, scale, floor = _gmm_case_resp(case)
    err = (r.cpu().double() - r64).abs().max().item() / scale
    tol = max(1e-4, 3.0 * floor)
    print("GMM_BWD resp_bits %s r: relative error %.3e, fp32 floor %.3e, bar %.3e" % ("-".join(map(str, case[:5])), err, floor, tol))
    assert err < tol, "r: relative error %.3e (fp32 floor %.3e, bar %.1e)" % (err, floor, tol)


def test_gmm_keyed_entry_with_host_built_tiles(L):
    """cf_gmm_logprob_keyed called directly: two scale keys x three mean keys (one pair without samples), seven tiles - two of one
    bucket (128 + 22 samples), one unused - over 768 columns, i.e. 12 slices: a serial sum of more than eight partials in
    the keyed finishing kernel, where the tree form would round differently.  Against gaussian.py:142-158 in fp64; the recorded bits."""
    from contextflow_amd.layers.distributions.gaussian import gmm_prepare
    from contextflow_amd.layers import _hip
    M, K, D, B, Us, Um = 10, 8, 768, 300, 2, 3
    MK = M * K
    g = torch.Generator().manual_seed(768300)
    mG, sG, wG = torch.randn(M, K, D, generator=g), 1 + 0.2 * torch.randn(M, K, D, generator=g), torch.randn(M, K, generator=g)
    cs, cm = 0.3 * torch.randn(Us, M, K, D, generator=g), 0.3 * torch.randn(Um, M, K, D, generator=g)
    x, out0 = torch.randn(B, D, generator=g), torch.randn(B, M, generator=g)
    perm = torch.randperm(B, generator=g)
    counts = {(0, 0): 150, (0, 1): 40, (0, 2): 0, (1, 0): 30, (1, 1): 50, (1, 2): 30}
    key_s, key_m = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    tiles, pos = [], 0
    for (ks, km), n in counts.items():                                     # order = perm: the samples grouped by (ks, km)
        key_s[perm[pos:pos + n]], key_m[perm[pos:pos + n]] = ks, km
        tiles += [[ks, km, pos + j, min(128, n - j)] for j in range(0, n, 128)]
        pos += n
    tiles.insert(3, [1, 2, 0, 0])                                          # an unused tile in the middle
    T = len(tiles)
    assert pos == B and T == 7 and sorted(t[3] for t in tiles)[:2] == [0, 22]
    preps = [gmm_prepare(mG.to(DEV), (sG + cs[ks]).to(DEV), wG.to(DEV)) for ks in range(Us)]
    a_tab = torch.stack([p[0] for p in preps]).contiguous()
    cst_tab = torch.stack([p[2] for p in preps]).contiguous()
    nm_tab = (-(mG.unsqueeze(0) + cm)).reshape(Um, MK, D).to(DEV)
    nbytes = _hip.lib().cf_gmm_keyed_ws_bytes(T, B, M, K, D)
    assert nbytes == 16 * B * MK * 4                                       # 16 slices of 48 columns asked for: 12 of 64 launched
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    xd, ks_d, tiles_d = x.to(DEV), key_s.to(DEV), torch.tensor(tiles, dtype=torch.int32).to(DEV)
    order_d = perm.to(torch.int32).to(DEV)

    def run(out, accumulate):
        _hip.call("cf_gmm_logprob_keyed", _hip.p(xd), _hip.p(a_tab), _hip.p(nm_tab), _hip.p(cst_tab), _hip.p(ks_d), _hip.p(tiles_d),
                  _hip.p(order_d), _hip.p(out), _hip.p(ws), T, B, M, K, D, D, accumulate, _hip.stream())
        return out
    ref = torch.empty(B, M, dtype=torch.float64)
    logw = torch.log_softmax(wG.double(), -1)
    for (ks, km), n in counts.items():
        idx = (key_s == ks) & (key_m == km)
        mu, sig = (mG + cm[km]).double(), torch.nn.functional.softplus((sG + cs[ks]).double())
        lp = (-0.5 * ((x[idx].double().view(-1, 1, 1, D) - mu) / sig) ** 2 - torch.log(sig) - 0.5 * math.log(2 * math.pi)).sum(-1)
        ref[idx] = torch.logsumexp(lp + logw, -1)
    scale = ref.abs().max().item()
    got = run(torch.empty(B, M, device=DEV), 0)
    _gmm_bits("keyed", (B, 0), [got])
    assert (got.cpu().double() - ref).abs().max().item() < 2e-6 * scale
    acc = run(out0.to(DEV), 1)
    _gmm_bits("keyed", (B, 1), [acc])
    assert (acc.cpu().double() - (out0.double() + ref)).abs().max().item() < 2e-6 * scale


@pytest.mark.parametrize("B,D,wide", [(1003, 768, 1536), (70, 1536, 1536), (4, 96, 128), (16384, 768, 768)])
def test_gmm_backward_sums_kernel(L, B, D, wide):
    """cf_gmm_bwd_sums (S0, S1, S2 of the mixture backward as one MFMA product over the batch, x read through its batch
    stride) against fp64 matmuls; ragged batch slices, a batch smaller than one k-step."""
    from contextflow_amd.layers import _hip
    g = torch.Generator().manual_seed(B + D)
    MK = 80
    xw = torch.randn(B, wide, generator=g).to(DEV)
    x = xw[:, wide - D:]
    r = torch.randn(B, MK, generator=g).to(DEV)
    lib = _hip.lib()
    assert lib.cf_gmm_bwd_sums_supported(MK, D) and not lib.cf_gmm_bwd_sums_supported(MK, D + 4) and not lib.cf_gmm_bwd_sums_supported(64, D)
    S0, S1, S2 = torch.empty(MK, device=DEV), torch.empty(MK, D, device=DEV), torch.empty(MK, D, device=DEV)
    ws = torch.empty(lib.cf_gmm_bwd_sums_ws_bytes(B, MK, D), device=DEV, dtype=torch.uint8)
    _hip.call("cf_gmm_bwd_sums", _hip.p(x), _hip.p(r), _hip.p(S0), _hip.p(S1), _hip.p(S2), _hip.p(ws), B, MK, D, wide, _hip.stream())
    rd, xd = r.double().cpu(), x.double().cpu()
    for got, want in ((S0, rd.sum(0)), (S1, rd.t() @ xd), (S2, rd.t() @ (xd * xd))):
        assert (got.cpu().double() - want).abs().max().item() <= 2e-6 * max(1.0, want.abs().max().item()) * max(1.0, (B / 1000) ** 0.5)


@pytest.mark.parametrize("onehot,K", [(1, 20), (0, 3), (1, 7)])
def test_grouped_linears_with_the_context_code_formed_in_the_kernel(L, onehot, K):
    """cf_linear_group: the first Linears of the CN nets of a specialist flow in one launch, the uniform dequantisation of the
    context (model.py:30-90, dequantize.py:55-64) formed while the input is staged; and plain grouped Linears.  Bitwise equal to
    cf_ctx_encode + cf_linear per problem (same tile, same summation order); ragged N, an empty and a 1-row batch."""
    from contextflow_amd.layers import _hip
    torch.manual_seed(3)
    for B in (0, 1, 301):
        cards = [15, 5] if K == 20 else ([3, 4] if onehot else [9, 4, 6])
        assert (sum(cards) if onehot else len(cards)) == K
        ctx = torch.stack([torch.randint(0, c, (B,)) for c in cards], 1).to(DEV)
        card = torch.tensor(cards, device=DEV)
        Ns, acts = [7, 96, 200, 33], [0, 2, 0, 2]
        n = len(Ns)
        us = [torch.rand(B, K, device=DEV) for _ in Ns]
        qs = [torch.rand(K, device=DEV) + 0.5 for _ in Ns]
        Ws = [torch.randn(N, K, device=DEV) for N in Ns]
        bs = [torch.randn(N, device=DEV) for N in Ns]
        ys = [torch.full((B, N), float("nan"), device=DEV) for N in Ns]
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts])
        iarr = lambda v: (ctypes.c_int * n)(*v)
        pp, st = _hip.p, _hip.stream()
        cs = [torch.full((B, K), float("nan"), device=DEV) if g != 1 else None for g in range(n)]      # the codes too (one problem without)
        _hip.call("cf_linear_group", n, arr(us), arr(qs), arr(Ws), arr(bs), arr(ys), arr(cs), iarr(Ns), iarr(acts), pp(ctx),
                  pp(card) if onehot else None, len(cards), onehot, B, K, st)
        xs = []
        for g in range(n):
            c = torch.empty(B, K, device=DEV)
            if B:
                _hip.call("cf_ctx_encode", pp(ctx), pp(us[g]), pp(qs[g]), pp(card) if onehot else None, pp(c), B, len(cards), K, onehot, st)
            want = torch.empty(B, Ns[g], device=DEV)
            _hip.call("cf_linear", pp(c), pp(Ws[g]), pp(bs[g]), None, pp(want), B, K, Ns[g], acts[g], st)
            assert torch.equal(ys[g], want), (B, g)
            assert cs[g] is None or torch.equal(cs[g], c), (B, g)
            xs.append(c)
        # plain grouped Linears (no context), one problem without a bias
        ys2 = [torch.full((B, N), float("nan"), device=DEV) for N in Ns]
        bs2 = [bs[0], None, bs[2], bs[3]]
        _hip.call("cf_linear_group", n, arr(xs), None, arr(Ws), arr(bs2), arr(ys2), None, iarr(Ns), iarr(acts), None, None, 0, 0, B, K, st)
        for g in range(n):
            want = torch.empty(B, Ns[g], device=DEV)
            _hip.call("cf_linear", pp(xs[g]), pp(Ws[g]), pp(bs2[g]), None, pp(want), B, K, Ns[g], acts[g], st)
            assert torch.equal(ys2[g], want), (B, g)


@pytest.mark.parametrize("C,H,W,B,cf,sq", [(16, 16, 16, 5, True, False), (16, 16, 16, 3, True, True), (32, 8, 8, 37, False, False),
                                            (32, 8, 8, 9, True, True), (64, 4, 4, 130, True, False), (64, 4, 4, 6, False, True),
                                            (8, 6, 6, 7, True, False), (12, 4, 4, 5, False, True),
                                            (76, 9, 8, 3, True, False), (76, 9, 8, 3, False, True)])      # > 64 KiB of LDS
def test_fused_specialist_affine_equals_its_two_layers(L, C, H, W, B, cf, sq):
    """cf_affine_ctx_fwd (per-sample Conv1x1 + per-sample ActNorm [+ Squeeze] in one pass; the one-wave-per-sample MFMA form at
    the three image-flow levels, the LDS form elsewhere) against Squeeze -> cf_conv1x1_ctx -> cf_actnorm_ctx and against
    conv1x1.py:34-50 / actnorm.py:40-60 in fp64; the log-det accumulates into a running buffer or assigns."""
    from contextflow_amd.layers import _hip
    from contextflow_amd.layers.squeeze import squeeze_op
    g = torch.Generator().manual_seed(C * 131 + H + B)
    r = lambda *sh: torch.randn(*sh, generator=g)
    HW = H * W
    xin = r(B, C // 4, 2 * H, 2 * W) if sq else r(B, C, H, W)
    wide = torch.cat([xin, r(*xin.shape)], 1).to(DEV)                        # the step input as a channel slice (SplitPrior view)
    xv = wide[:, : xin.shape[1]]
    m1, m2 = 0.3 * r(B, C * C), 0.3 * r(B, 2 * C)
    Wm = torch.linalg.qr(r(C, C))[0].contiguous() if cf else None
    t, logs = (0.2 * r(C), 0.2 * r(C)) if cf else (None, None)
    lad, cadd = (r(1) if cf else None), 0.375
    d = lambda v: None if v is None else v.to(DEV).contiguous()
    P, st = _hip.p, _hip.stream()
    # reference chain on the GPU
    xs = squeeze_op(xv, (2, 2), False) if sq else xv
    xs, xbs = _hip.bview(xs)
    z1, l1 = torch.empty(B, C, H, W, device=DEV), torch.empty(B, device=DEV)
    _hip.call("cf_conv1x1_ctx", P(xs), P(d(m1)), P(d(Wm)), P(z1), P(l1), B, C, HW, xbs, st)
    z2, l2 = torch.empty_like(z1), torch.empty(B, device=DEV)
    _hip.call("cf_actnorm_ctx", P(z1), P(d(m2)), P(d(t)), P(d(logs)), P(z2), P(l2), B, C, HW, C * HW, st)
    want_l = l1 + l2 + cadd + (HW * lad.item() if cf else 0.0)
    for accumulate in (0, 1):
        z = torch.full((B, C, H, W), float("nan"), device=DEV)
        ldj = torch.full((B,), 2.5, device=DEV)
        _hip.call("cf_affine_ctx_fwd", P(xv), P(d(m1)), P(d(Wm)), P(d(m2)), P(d(t)), P(d(logs)), P(d(lad)), cadd, P(z), P(ldj), B, C, H, W,
                  wide.stride(0), int(sq), accumulate, 0, st)
        assert (z - z2).abs().max().item() <= 2e-5 * max(1.0, z2.abs().max().item())
        assert (ldj - (want_l + (2.5 if accumulate else 0.0))).abs().max().item() <= 2e-5 * max(1.0, want_l.abs().max().item())
    # blocked form of m1 (the 16 x 16 blocks on and below the diagonal only): same bits as the dense form
    nblk = _hip.lib().cf_affine_ctx_blocked_floats(C, H, W)
    assert (nblk > 0) == ((C, H, W) in ((16, 16, 16), (32, 8, 8), (64, 4, 4)))
    if nblk:
        from contextflow_amd.layers.specialist import blocked_rows
        idx = torch.tensor(blocked_rows(C))
        assert idx.numel() == nblk
        zb, lb_ = torch.full((B, C, H, W), float("nan"), device=DEV), torch.empty(B, device=DEV)
        _hip.call("cf_affine_ctx_fwd", P(xv), P(d(m1[:, idx])), P(d(Wm)), P(d(m2)), P(d(t)), P(d(logs)), P(d(lad)), cadd, P(zb), P(lb_), B, C,
                  H, W, wide.stride(0), int(sq), 0, 1, st)
        zd, ld_ = torch.empty_like(zb), torch.empty(B, device=DEV)
        _hip.call("cf_affine_ctx_fwd", P(xv), P(d(m1)), P(d(Wm)), P(d(m2)), P(d(t)), P(d(logs)), P(d(lad)), cadd, P(zd), P(ld_), B, C, H, W,
                  wide.stride(0), int(sq), 0, 0, st)
        assert torch.equal(zb, zd) and torch.equal(lb_, ld_)
    # fp64 formula
    xd = (squeeze_op(xv, (2, 2), False) if sq else xv).double().cpu().reshape(B, C, HW)
    M1 = m1.double().view(B, C, C)
    Wb = torch.tril(M1, -1) + torch.diag_embed(torch.exp(torch.diagonal(M1, dim1=1, dim2=2)))
    if cf:
        Wb = Wb + Wm.double() - torch.eye(C, dtype=torch.float64)
    tb = m2[:, :C].double() + (t.double() if cf else 0.0)
    lb = m2[:, C:].double() + (logs.double() if cf else 0.0)
    ref = (torch.bmm(Wb, xd) - tb[:, :, None]) * torch.exp(-lb)[:, :, None]
    assert (z.double().cpu().reshape(B, C, HW) - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("rows", [1, 37, 1000, 20000])
def test_grouped_linear_weight_gradients_against_matmul(L, rows):
    """cf_linear_wgrad_group (cf_rowgemm.hip: 16x16 MFMA tiles fed from global memory, one wave per tile group and row range)
    against fp64 matmuls: widths that are not multiples of 16, more than 6 x 4 tiles per member, a ragged last k-step, members
    with and without bias."""
    from contextflow_amd.layers.autograd import wgrad_group
    g = torch.Generator().manual_seed(rows)
    shapes = [(26, 26), (26, 52), (52, 192), (64, 52), (52, 52), (5, 7), (130, 100), (1, 200)]        # (K, N)
    members, refs = [], []
    for i, (K, N) in enumerate(shapes):
        x, gy = torch.randn(rows, K, generator=g), torch.randn(rows, N, generator=g)
        members.append((x.to(DEV), gy.to(DEV), i % 2 == 0))
        refs.append((gy.double().t() @ x.double(), gy.double().sum(0)))
    res = wgrad_group(members, torch.device(DEV))
    tol = 3e-6 * max(1.0, (rows / 100) ** 0.5)
    for (gW, gb), (rW, rb), m in zip(res, refs, members):
        assert (gW.double().cpu() - rW).abs().max().item() <= tol * max(1.0, rW.abs().max().item())
        assert (gb is not None) == m[2]
        if gb is not None:
            assert (gb.double().cpu() - rb).abs().max().item() <= tol * max(1.0, rb.abs().max().item())
    again = wgrad_group(members, torch.device(DEV))                          # fixed summation order: bitwise repeatable
    for (a, _), (b, _) in zip(res, again):
        assert torch.equal(a, b)


def test_preprocessing(L):
    t, _ = unit("normalize")
    n = L.Normalization(translation=1e-4, scale=1 / (1 - 2e-4)).to(DEV)
    z, ldj = n(t["x"].to(DEV))
    close(z, t["z"], tol=1e-7); close(ldj, t["ldj"], tol=1e-6)
    close(n.reverse(t["z"].to(DEV)), t["xrec"], tol=1e-6)
    t, _ = unit("normalize256")
    z, ldj = L.Normalization(translation=0.0, scale=256.0).to(DEV)(t["x"].to(DEV))
    close(z, t["z"], tol=1e-7); close(ldj, t["ldj"], tol=1e-6)
    t, _ = unit("logit")
    lt = L.LogitTransform()
    z, ldj = lt(t["x"].to(DEV))
    close(z, t["z"], tol=1e-6); close(ldj, t["ldj"], tol=1e-6)
    close(lt.reverse(t["z"].to(DEV)), t["xrec"], tol=1e-6)
    t, _ = unit("stdnormal")
    close(L.StandardNormal((1, 4, 4)).to(DEV).log_prob(t["x"].to(DEV)), t["logp"], tol=1e-6)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("tag", ["trans_ts", "trans_img"])
def test_transcoupling(L, tag, fused):
    t, sd = unit(tag)
    sz = tuple(int(v) for v in t["in_sz"]); patch = tuple(int(v) for v in t["p"])
    m = L.TransCoupling(sz, patch)
    m.load_state_dict(sd)
    m = m.to(DEV)
    m.fused = fused
    x = t["x"].to(DEV)
    assert m._fused_ok(x) == fused
    close(m.net(x[:, : sz[0] // 2]), t["h"], tol=2e-5)
    z, ldj = m(x)
    close(z, t["z"], tol=2e-5); close(ldj, t["ldj"], tol=2e-5)
    close(m.reverse(t["z"].to(DEV)), t["xrec"], tol=1e-4)


@pytest.mark.parametrize("variant", ["wave", "rs"])
@pytest.mark.parametrize("B", [3, 37])
def test_vit_step_kernel(L, B, variant):
    """Conv1x1 -> ActNorm -> TransCoupling as ONE kernel (SMAP geometry), in both forms of cf_vit_step_fwd - 'wave' (register-resident,
    8 samples per wave) and 'rs' (row-split over the four waves of a workgroup, 4 samples per workgroup): with an
    identity Conv1x1 / ActNorm it must reproduce the reference's TransCoupling vectors (conditioner output h, z, log-det);
    with random ones, the composition of the three oracle layers at a ragged batch (last wave partly filled)."""
    from contextflow_amd.layers import _hip
    t, sd = unit("trans_ts")
    sz = tuple(int(v) for v in t["in_sz"]); patch = tuple(int(v) for v in t["p"])
    C = sz[0]
    m = L.TransCoupling(sz, patch)
    m.load_state_dict(sd)
    m = m.to(DEV)
    assert m.step_supported(sz)
    # identity front: the layer alone against the reference's own output
    x = t["x"].to(DEV)
    tables = m.step_tables([(m, torch.eye(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV))], torch.device(DEV), variant)[0]
    ld = torch.zeros(x.shape[0], device=DEV)
    h = torch.full_like(x, float("nan"))
    z = m.step_forward(x, tables, ld, h_out=h)
    close(h, t["h"], tol=2e-5); close(z, t["z"], tol=2e-5); close(ld, t["ldj"], tol=2e-5)
    # random Conv1x1 / ActNorm in front, ragged batch, accumulation into a non-zero running log-det
    g = torch.Generator().manual_seed(B)
    Wm = torch.linalg.qr(torch.randn(C, C, generator=g))[0] + 0.1 * torch.randn(C, C, generator=g)
    tt, logs = 0.3 * torch.randn(C, generator=g), 0.4 * torch.randn(C, generator=g)
    xx = torch.randn(B, *sz, generator=g)
    p = {"0." + k: v for k, v in sd.items()}
    y, l0 = fo.conv1x1_fwd(xx, Wm)
    y, l1 = fo.actnorm_fwd(y, tt, logs)
    zref, l2 = fo.transcoupling_fwd(y, p, "0.", sz, patch)
    tables = m.step_tables([(m, Wm.to(DEV), tt.to(DEV), logs.to(DEV))], torch.device(DEV), variant)[0]
    ld = torch.full((B,), 1.5, device=DEV)
    z = m.step_forward(xx.to(DEV), tables, ld)
    close(z, zref, tol=2e-5)
    close(ld, 1.5 + l0 + l1 + l2, tol=2e-5)


@pytest.mark.parametrize("form", ["wave", "rs"])
def test_vit_step_tables_batched_equal_single(L, form):
    """TransCoupling.step_tables on 17 SMAP-geometry steps at once packs, bit for bit, what 17 calls with one step each pack:
    17 is the smallest count that crosses the 16-step chunk of the batched pack kernels (the `+ i0` offsets of the Wm^-1 and
    backward-table arrays can go wrong only there).  Row-split form: with Wm^-1 and the backward kernel's tables."""
    t, sd = unit("trans_ts")
    sz = tuple(int(v) for v in t["in_sz"]); patch = tuple(int(v) for v in t["p"])
    C, dev = sz[0], torch.device(DEV)
    items = []
    for i in range(17):
        g = torch.Generator().manual_seed(100 + i)
        m = L.TransCoupling(sz, patch)
        m.load_state_dict({k: v + 0.05 * torch.randn(v.shape, generator=g) if v.is_floating_point() else v for k, v in sd.items()})
        Wm = torch.linalg.qr(torch.randn(C, C, generator=g))[0] + 0.1 * torch.randn(C, C, generator=g)
        items.append((m.to(DEV), Wm.to(DEV), (0.3 * torch.randn(C, generator=g)).to(DEV), (0.4 * torch.randn(C, generator=g)).to(DEV)))
    train = form == "rs"
    batched = L.TransCoupling.step_tables(items, dev, form, winv=train, bwd=train)
    single = [L.TransCoupling.step_tables([it], dev, form, winv=train, bwd=train)[0] for it in items]
    torch.cuda.synchronize()

    def bits(ws):            # floats 2 and 3 of a forward table's header are padding: no kernel writes or reads them
        v = ws.view(torch.int32).clone()
        v[2:4] = 0
        return v
    assert len(batched) == len(single) == 17
    for i, (a, b) in enumerate(zip(batched, single)):
        assert a.form == b.form == form
        assert torch.equal(bits(a.ws), bits(b.ws)), i
        if train:
            assert torch.equal(a.winv.view(torch.int32), b.winv.view(torch.int32)), i
            assert torch.equal(a.wsb.view(torch.int32), b.wsb.view(torch.int32)), i
        else:
            assert a.winv is None and a.wsb is None
    assert not torch.equal(bits(batched[0].ws), bits(batched[16].ws))          # (different parameters per step)


# ------------------------------------------------------------------------------------------ fused step kernel
@pytest.mark.parametrize("squeeze", [False, True])
@pytest.mark.parametrize("C,H,W,B", [(16, 16, 16, 3), (32, 8, 8, 5), (64, 4, 4, 11), (8, 16, 16, 2), (32, 8, 8, 8), (64, 4, 4, 16)])
def test_fused_step_phases(L, C, H, W, B, squeeze):
    """Conv1x1->ActNorm->Coupling in one MFMA kernel, every intermediate plane against the oracle
    (ragged batch sizes exercise the partially filled last workgroup)."""
    from tests.gpu_util import fused_step_debug
    torch.manual_seed(C * 1000 + B)
    conv, act, cpl = L.Conv1x1((C, H, W)), L.ActNorm((C, H, W)), L.Coupling(C, kernel_size=(3, 3), padding=(1, 1))
    with torch.no_grad():
        conv.NN.add_(0.1 * torch.randn(C, C))
        act.NN_t.copy_(0.3 * torch.randn(C)); act.NN_logs.copy_(0.2 * torch.randn(C)); act.initialized.fill_(1)
    act._init_done = True
    x = torch.randn(B, C, H, W)
    # oracle
    p = {"0." + k: v.detach() for k, v in cpl.state_dict().items()}
    y, l0 = fo.conv1x1_fwd(x, conv.NN.detach())
    y, l1 = fo.actnorm_fwd(y, act.NN_t.detach(), act.NN_logs.detach())
    h1 = torch.relu(torch.nn.functional.conv2d(y[:, : C // 2], p["0.NN.0.weight"], p["0.NN.0.bias"]))
    h2 = torch.relu(torch.nn.functional.conv2d(torch.nn.functional.pad(h1, (1, 1, 1, 1), mode="reflect"),
                                               p["0.NN.2.weight"], p["0.NN.2.bias"]))
    h = torch.nn.functional.conv2d(h2, p["0.NN.4.weight"], p["0.NN.4.bias"])
    zref, l2 = fo.coupling_apply_fwd(y, h)
    for m in (conv, act, cpl):
        m.to(DEV)
    xin = fo.squeeze_inv(x, (2, 2)) if squeeze else x          # feed the un-squeezed tensor: Squeeze is folded in
    z, ldj, d = fused_step_debug(xin.to(DEV).contiguous(), conv, act, cpl, squeeze=squeeze)
    close(d["y0"], y[:, : C // 2]); close(d["h1"], h1); close(d["h2"], h2); close(d["h"], h)
    close(z, zref)
    close(ldj, l0 + l1 + l2, tol=1e-5)
    if H == 16:                                            # 16x16 images: every plane of k_flow_step_small as well
        z, ldj, d2 = fused_step_debug(xin.to(DEV).contiguous(), conv, act, cpl, squeeze=squeeze, variant=3)
        close(d2["y0"], y[:, : C // 2]); close(d2["h1"], h1); close(d2["h2"], h2); close(d2["h"], h)
        close(z, zref)
        close(ldj, l0 + l1 + l2, tol=1e-5)
    close(d["z_prod"], zref)                               # cf_flow_step_fwd: the kernel variant production picks
    close(d["ldj_prod"], l0 + l1 + l2, tol=1e-5)


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("name", ["mnist", "cifar10", "smap", "atm"])
@pytest.mark.parametrize("fused", [False, True])
def test_e2e_golden(L, name, fused):
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e(name)
    x, u, eps = e2e_inputs(name, fx)
    model = build_model(name, params)
    model.fused = fused
    set_noise(model, u, eps)
    z, logp = model(x.to(DEV), torch.zeros(x.shape[0], 1, dtype=torch.long, device=DEV))
    ref = torch.from_numpy(fx["logp"])
    d = (bpd(logp.cpu(), name) - bpd(ref, name)).abs().max().item()
    assert d < BPD_TOL, "bits/dim differ by %.3e" % d
    D = np.prod(fo.CONFIGS[name][0])
    assert (logp.cpu() - ref).abs().max().item() / (D * math.log(2)) < BPD_TOL
    close(z, torch.from_numpy(fx["z"]), tol=2e-5)
    assert (model.log_prob(x.to(DEV)).cpu() - logp.cpu()).abs().max() == 0     # deterministic given the noise


@pytest.fixture
def smap_step_form(request):
    """Forces one of the two forms of the one-kernel transformer step (cf_vit_step_fwd: 'rs' | 'wave')
    whatever the batch size; None = the production dispatch (TransCoupling.step_variant)."""
    from contextflow_amd.layers.coupling import TransCoupling
    form = getattr(request, "param", None)
    old = TransCoupling.STEP_RS_MAX_BATCH
    if form is not None:
        TransCoupling.STEP_RS_MAX_BATCH = {"rs": 1 << 40, "wave": 0}[form]
    yield form
    TransCoupling.STEP_RS_MAX_BATCH = old


@pytest.mark.parametrize("smap_step_form", ["rs", "wave"], indirect=True)
@pytest.mark.parametrize("tag", [None, "stress", "extreme"])
def test_e2e_smap_fixtures_through_each_step_form(L, tag, smap_step_form):
    """Both one-kernel forms of the transformer step on the reference's fixtures at the fixture batch (4 / 64 / 8 samples):
    the production dispatch would send all of them to the row-split form, so the wave form - the kernel behind the SMAP
    benchmark line - is forced through the same inputs and held to the same bars."""
    from tests.gpu_util import build_model, set_noise
    from contextflow_amd.layers.coupling import TransCoupling
    ops, _, M, params, fx = load_e2e("smap", tag)
    x, u, eps = e2e_inputs("smap", fx)
    tol = stress_tolerance(fx, tag) if tag else BPD_TOL
    model = build_model("smap", params)
    assert all(m.step_variant(x.shape[0]) == smap_step_form for m in model.sequence_modules if isinstance(m, TransCoupling))
    set_noise(model, u, eps)
    with torch.no_grad():
        z, logp = model(x.to(DEV))
    ref, ref64 = torch.from_numpy(fx["logp"]), torch.from_numpy(fx["logp_f64"])
    d32 = (bpd(logp.cpu(), "smap") - bpd(ref, "smap")).abs().max().item()
    d64 = (bpd(logp.cpu(), "smap") - bpd(ref64, "smap")).abs().max().item()
    print("smap %s %s: |d bits/dim| vs reference fp32 %.2e, vs its fp64 run %.2e (bar %.1e)" % (tag, smap_step_form, d32, d64, tol))
    assert d32 < tol and d64 < tol, (d32, d64, tol)
    zr = torch.from_numpy(fx["z"])
    assert (z.cpu() - zr).abs().max().item() <= 2e-4 * max(1.0, zr.abs().max().item())


@pytest.mark.parametrize("tag", ["stress", "extreme"])
@pytest.mark.parametrize("name", ["mnist", "cifar10", "smap"])
@pytest.mark.parametrize("fused", [False, True])
def test_e2e_stress_regimes(L, name, fused, tag):
    """Trained-like parameter regimes (tests/golden/make_golden.py: end_to_end_stress) against the reference's own
    output: coupling raw log-scales up to +-25 (tanh saturated), ActNorm log-scales of -4.7 .. +5, Conv1x1 of condition
    number 1e3, mixture sigmas 0.13 .. 6 ("stress", B = 64, bar 1e-5 bits/dim) or 0.018 .. 6 with |raw| up to 27
    ("extreme": bar = max(1e-5, 1.5x the reference's own fp32-vs-fp64 distance, stored in the fixture))."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e(name, tag)
    x, u, eps = e2e_inputs(name, fx)
    tol = stress_tolerance(fx, tag)
    model = build_model(name, params)
    model.fused = fused
    set_noise(model, u, eps)
    z, logp = model(x.to(DEV))
    ref, ref64 = torch.from_numpy(fx["logp"]), torch.from_numpy(fx["logp_f64"])
    d32 = (bpd(logp.cpu(), name) - bpd(ref, name)).abs().max().item()
    d64 = (bpd(logp.cpu(), name) - bpd(ref64, name)).abs().max().item()
    print("%s %s fused=%s: |d bits/dim| vs reference fp32 %.2e, vs reference fp64 %.2e (reference fp32 vs fp64 %.2e)"
          % (name, tag, fused, d32, d64, float(fx["floor_bpd"])))
    assert d32 < tol and d64 < tol, (d32, d64, tol)
    zr = torch.from_numpy(fx["z"])
    assert (z.cpu() - zr).abs().max().item() <= 2e-4 * max(1.0, zr.abs().max().item())
    # first call on un-initialised ActNorms (init on ill-conditioned Conv1x1 outputs), then the fused plan.  The exact answer
    # for THIS call is the fp64 oracle initialising from the same batch: the build's statistics are fp64 sums, the reference's
    # are fp32 `mean` / `std`, and in these regimes that difference alone moves the log-density (d_init below: the fp64 oracle
    # with its own init against the fp64 reference run with the reference's init - 3.9e-6 bits/dim on cifar10 and 3.0e-6 on smap "extreme").
    # So: within the bar of the exact first-call answer, and within bar + d_init of the reference's fp32 first call.
    pre = pre_init_params(name, fx)
    pre64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in pre.items()}
    _, lp64_first = fo.flow_forward(ops, pre64, x.double(), None if u is None else u.double(), [e.double() for e in eps], init_actnorm=True)
    d_init = (bpd(lp64_first, name) - bpd(ref64, name)).abs().max().item()
    model = build_model(name, pre)
    model.fused = fused
    set_noise(model, u, eps)
    for call in ("first (initialising)", "second (fused plan)"):
        _, lp = model(x.to(DEV))
        e64 = (bpd(lp.cpu(), name) - bpd(lp64_first, name)).abs().max().item()
        e32 = (bpd(lp.cpu(), name) - bpd(ref, name)).abs().max().item()
        print("%s %s fused=%s %s call: %.2e from the exact first-call answer, %.2e from the reference's fp32 (its init moves it by %.2e)"
              % (name, tag, fused, call, e64, e32, d_init))
        assert e64 < tol and e32 < tol + d_init, (call, e64, e32, d_init, tol)


@pytest.mark.parametrize("name", ["mnist", "cifar10", "smap", "atm"])
def test_e2e_actnorm_first_call(L, name):
    """First call on un-initialised ActNorms reproduces the reference's data-dependent init."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, post, fx = load_e2e(name)
    x, u, eps = e2e_inputs(name, fx)
    model = build_model(name, pre_init_params(name, fx))
    set_noise(model, u, eps)
    _, logp = model(x.to(DEV))
    sd = model.state_dict()
    for k in post:
        if k.endswith(("NN_t", "NN_logs")):
            assert torch.allclose(sd[k].cpu(), post[k], rtol=1e-4, atol=2e-5), k
        if k.endswith("initialized"):
            assert int(sd[k]) == 1
    assert (bpd(logp.cpu(), name) - bpd(torch.from_numpy(fx["logp"]), name)).abs().max() < BPD_TOL
    _, logp2 = model(x.to(DEV))                       # second call takes the fused plan
    assert (bpd(logp2.cpu(), name) - bpd(torch.from_numpy(fx["logp"]), name)).abs().max() < BPD_TOL


def test_state_dict_roundtrip_and_trace(L):
    """Per-layer ldj / activations of the layer-by-layer mode against the reference trace (cifar10)."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e("cifar10")
    x, u, eps = e2e_inputs("cifar10", fx)
    model = build_model("cifar10", params)
    set_noise(model, u, eps)
    h = x.to(DEV)
    for i, m in enumerate(model.sequence_modules):
        h, ldj = m(h, None)
        r = torch.from_numpy(fx["ldj%d" % i])
        assert ldj.shape == r.shape, (i, type(m).__name__)
        assert torch.allclose(ldj.cpu(), r, rtol=3e-6, atol=3e-3), (i, type(m).__name__, (ldj.cpu() - r).abs().max())
        if "z%d" % i in fx:
            close(h, torch.from_numpy(fx["z%d" % i]), tol=2e-5)


# ------------------------------------------------------------------------------------------ full-size properties
@pytest.mark.parametrize("name,B", [("cifar10", 2048), ("mnist", 2048), ("smap", 4096)])
def test_full_size_properties(L, name, B):
    """At benchmark batch sizes the oracle is too slow for every sample, so use size-independent
    properties: (1) per-sample results do not depend on the batch they are computed in (a slice
    re-run alone and checked against the oracle), (2) fused plan == layer-by-layer mode,
    (3) permuting the batch permutes the output."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e(name)
    model = build_model(name, params)
    g = torch.Generator().manual_seed(5)
    C, H, W = fo.CONFIGS[name][0]
    x = torch.rand(B, C, H, W, generator=g) if name == "smap" else torch.randint(0, 256, (B, C, H, W), generator=g).float()
    u = torch.rand(B, C, H, W, generator=g) if name != "smap" else None
    eps = [torch.randn(B, 1, H, W, generator=g)]
    set_noise(model, u, eps)
    torch.set_grad_enabled(False)                       # evaluation throughout, as in experiment_cl.py:163-185
    try:
        _full_size_checks(model, name, B, ops, params, x, u, eps, g)
    finally:
        torch.set_grad_enabled(True)


def _full_size_checks(model, name, B, ops, params, x, u, eps, g):
    from tests.gpu_util import set_noise
    _, logp = model(x.to(DEV))
    assert torch.isfinite(logp).all()
    model.fused = False
    _, logp_layers = model(x.to(DEV))
    model.fused = True
    D = np.prod(fo.CONFIGS[name][0]) * math.log(2)
    # (2) both execution modes against the EXACT answer - the fp64 oracle on all B samples - at the bits/dim bar.  This replaces
    # round 3's fused-vs-layers self-comparison at 2 x the bar: two fp32 evaluations that each sit within the bar of the exact
    # answer are within twice the bar of each other and no closer in general - on 4096 SMAP samples the reference's own fp32
    # arithmetic is 7.8e-6 from its fp64 run on the worst sample (rms 8.9e-7), the one-kernel steps 5.3e-6 (row-split) and
    # 8.2e-6 (wave), the layer kernel 7.4e-6, all with the same rms (profiles/r4_vit_step_wave.md, section 3): the tail belongs to the
    # samples with |logp| ~ 1500 nats, where one ulp of logp is already 9e-7 bits/dim.
    p64 = {k: (v.double() if v.is_floating_point() else v) for k, v in params.items()}
    _, ref64 = fo.flow_forward(ops, p64, x.double(), None if u is None else u.double(), [eps[0].double()])
    for mode, lp in (("fused", logp), ("layers", logp_layers)):
        e = (bpd(lp.cpu(), name) - bpd(ref64, name)).abs()
        print("%s B=%d %s vs the fp64 oracle: max %.2e rms %.2e bits/dim" % (name, B, mode, e.max(), e.pow(2).mean().sqrt()))
        assert e.max().item() < BPD_TOL, (mode, e.max().item())
    assert (logp - logp_layers).abs().max().item() / D < 2 * BPD_TOL          # (follows from the two above)
    # (1) a ragged slice alone + oracle on it
    sl = slice(B - 37, B - 4)
    set_noise(model, None if u is None else u[sl], [eps[0][sl]])
    _, lp_slice = model(x[sl].to(DEV))
    # (the mixture kernels split the feature dimension over more workgroups for small batches: another summation order,
    # a few ulp of |logp| ~ 6e3)
    assert (lp_slice - logp[sl]).abs().max().item() / D < 3e-6
    _, ref = fo.flow_forward(ops, params, x[sl], None if u is None else u[sl], [eps[0][sl]])
    assert (bpd(lp_slice.cpu(), name) - bpd(ref, name)).abs().max() < BPD_TOL
    # (3) permutation equivariance
    perm = torch.randperm(B, generator=g)
    set_noise(model, None if u is None else u[perm], [eps[0][perm]])
    _, lp_perm = model(x[perm].to(DEV))
    assert (lp_perm.cpu() - logp.cpu()[perm]).abs().max().item() / D < 1e-6


def test_roundtrip_layers_full_size(L):
    """reverse(forward(x)) == x for the invertible layers at benchmark sizes (cifar10 level shapes)."""
    torch.manual_seed(0)
    for C, H, W in ((16, 16, 16), (32, 8, 8), (64, 4, 4)):
        B = 1024
        x = torch.randn(B, C, H, W, device=DEV)
        conv, act, cpl = L.Conv1x1((C, H, W)).to(DEV), L.ActNorm((C, H, W)).to(DEV), L.Coupling(C, (3, 3), (1, 1)).to(DEV)
        for m in (conv, act, cpl):
            z, _ = m(x)
            close(m.reverse(z), x, tol=2e-5)
        sq = L.Squeeze((2, 2))
        assert torch.equal(sq.reverse(sq(x)[0]), x)


# ------------------------------------------------------------------------------------------ ABI behaviour
def test_abi_errors(L):
    from contextflow_amd.layers import _hip
    lib = _hip.lib()
    rc = lib.cf_squeeze(None, None, 1, 1, 2, 2, 2, 2, 4, 4, 0, None)
    assert rc == -1 and b"cf_squeeze" in lib.cf_last_error()
    assert lib.cf_flow_step_supported(12, 6, 10, 3, 3) == 0
    with pytest.raises(RuntimeError):
        L.Squeeze((2, 2))(torch.zeros(1, 1, 2, 2))           # CPU tensor: no fallback
    # empty batches: every batched entry point returns 0 without touching its (null) pointers
    N = None
    assert lib.cf_flow_step_fwd_taped(N, N, N, N, N, N, N, N, 0, 16, 16, 16, 4096, 0, N) == 0
    assert lib.cf_flow_step_bwd_taped(N, N, N, N, N, N, N, N, N, 0, 16, 16, 16, 0, N) == 0
    assert lib.cf_flow_step_fwd_ctx_taped(N, N, N, N, N, N, N, N, N, 0, 16, 16, 16, 4096, N) == 0
    assert lib.cf_gmm_ctx_logprob(N, N, N, N, N, N, N, 0, 2, 2, 4, 16, 64, 0, N) == 0
    assert lib.cf_gmm_ctx_logprob_tab(N, N, N, N, N, N, N, N, N, N, 0, 2, 2, 4, 16, 64, 0, N) == 0
    assert lib.cf_gmm_ctx_bwd(N, N, N, N, N, N, N, N, N, 0, 2, 2, 4, 16, 64, N) == 0
    assert lib.cf_gmm_ctx_bwd_tab(N, N, N, N, N, N, N, N, N, N, N, N, 0, 2, 2, 4, 16, 64, N) == 0
    assert lib.cf_gmm_ctx_pgrad_tab(N, N, N, N, N, N, N, N, N, 0, 2, 2, 4, 16, 64, 256, N) == 0
    assert lib.cf_gmm_ctx_tables(N, N, N, N, N, 0, 4, 4, 16, N) == 0
    assert lib.cf_conv1x1_ctx(N, N, N, N, N, 0, 16, 64, 1024, N) == 0
    assert lib.cf_conv1x1_ctx_bwd(N, N, N, N, N, N, N, 0, 16, 64, 1024, 1024, N) == 0
    assert lib.cf_linear(N, N, N, N, N, 0, 8, 8, 0, N) == 0
    assert lib.cf_activation(N, N, N, 0, 8, 2, 0.3, 0.0, N, 0, N) == 0
    assert lib.cf_attention(N, N, 0, 4, 64, 0.125, N) == 0
    # shapes outside a kernel's range are refused with a message, not launched
    assert lib.cf_slogdet_inverse(ctypes.c_void_p(16), 193, ctypes.c_void_p(16), N, N) == -2 and b"193" in lib.cf_last_error()
    # the transformer step backward: depth outside 1 .. 6 and channel counts other than 26 (host-side argument checks)
    q = ctypes.c_void_p(16)
    for depth in (0, 7):
        assert lib.cf_vit_step_bwd(q, q, q, q, q, q, q, q, N, 4, 26, depth, 26 * 8, N) == -1 and b"cf_vit_step_bwd" in lib.cf_last_error()
        assert lib.cf_vit_step_bwd_prepare_batch(0, q, q, q, q, 26, depth, N) == -1 and b"cf_vit_step_bwd_prepare_batch" in lib.cf_last_error()
    assert lib.cf_vit_step_bwd(q, q, q, q, q, q, q, q, N, 4, 24, 6, 24 * 8, N) == -2 and b"C=24" in lib.cf_last_error()
    assert lib.cf_vit_step_bwd_prepare_batch(0, q, q, q, q, 24, 6, N) == -2 and b"C=24" in lib.cf_last_error()
    assert lib.cf_vit_step_bwd_prepare_batch(0, q, q, q, q, 26, 6, N) == 0


@pytest.mark.parametrize("tag,indiv", [("spline_shared", False), ("spline_indiv", True)])
def test_spline_activation(L, tag, indiv):
    t, sd = unit(tag)
    m = L.SplineActivation((3, 4, 5), n_bins=5, tail_bound=10., individual_weights=indiv)
    m.load_state_dict(sd)
    m = m.to(DEV)
    z, ldj = m(t["x"].to(DEV))
    close(z, t["z"]); close(ldj, t["ldj"])
    close(m.reverse(t["z"].to(DEV)), t["xrec"])
    close(m.reverse(z), t["x"], tol=2e-5)
    close(m.logdet(t["x"].to(DEV)), t["ldj"])
    # full size, size-independent properties: round trip, monotone, identity outside the tails
    g = torch.Generator().manual_seed(2)
    x = (8.0 * torch.randn(4096, 3, 4, 5, generator=g)).to(DEV)
    z, ldj = m(x)
    close(m.reverse(z), x, tol=5e-5)
    out = x.abs() > 10.0
    assert out.any() and torch.equal(z[out], x[out]) and torch.isfinite(ldj).all()


@pytest.mark.parametrize("C,H,W,B", [(16, 16, 16, 3), (32, 8, 8, 5), (64, 4, 4, 21), (8, 16, 16, 2)])
def test_fused_inverse_step(L, C, H, W, B):
    """cf_flow_step_inv against the oracle's layer inverses, and forward(inverse(z)) == z through the fused pair.
    A smoke-sized check: 2 to 21 samples, Gaussian z, near-identity parameters, the fp32 oracle at 3e-5 of scale.  It does not
    cover production batches and their partly filled last workgroup, a batch-strided z, the direct form of the conditioner or
    trained-like parameters: tests/test_sampling.py holds the kernel to 1e-5 of scale against fp64 on all of those."""
    import contextflow_amd as cfa
    torch.manual_seed(C + B)
    conv, act, cpl = L.Conv1x1((C, H, W)), L.ActNorm((C, H, W)), L.Coupling(C, kernel_size=(3, 3), padding=(1, 1))
    with torch.no_grad():
        conv.NN.add_(0.1 * torch.randn(C, C))
        act.NN_t.copy_(0.3 * torch.randn(C)); act.NN_logs.copy_(0.2 * torch.randn(C)); act.initialized.fill_(1)
    act._init_done = True
    z = torch.randn(B, C, H, W)
    p = {"0." + k: v.detach() for k, v in cpl.state_dict().items()}
    ref = fo.coupling_inv(z, p, "0.", (1, 1))
    ref = fo.actnorm_inv(ref, act.NN_t.detach(), act.NN_logs.detach())
    ref = fo.conv1x1_inv(ref, conv.NN.detach())
    flow = cfa.layers.FlowSequential(L.GaussianMixtureDistribution(size=(C, H, W), mixtures=2, components=8), conv, act, cpl).to(DEV)
    x = flow.inverse(z.to(DEV))
    close(x, ref, tol=3e-5)
    flow.fused = False
    close(flow.inverse(z.to(DEV)), ref, tol=3e-5)           # layer-by-layer inverse agrees too
    flow.fused = True
    zz = x
    for m in flow.sequence_modules:
        zz, _ = m(zz)
    close(zz, z, tol=5e-5)
    # a Squeeze((2,2)) in front of the step: its reverse is folded into the inverse kernel's stores (x_unsqueezed) - the very
    # same numbers as the layer-by-layer inverse, in the layout of the tensor before the Squeeze
    if C % 4 == 0:
        flow2 = cfa.layers.FlowSequential(flow.dist, L.Squeeze((2, 2)), conv, act, cpl).to(DEV)
        xs = flow2.inverse(z.to(DEV))
        assert tuple(xs.shape) == (B, C // 4, 2 * H, 2 * W)
        assert torch.equal(xs, L.Squeeze((2, 2)).reverse(x))


# ------------------------------------------------------------------------------------------ sampling direction
def test_inverse_chain_mnist_golden(L):
    """FlowSequential.sample's layer chain (flowsequential.py:32-39) on the reference's own z -> x vectors."""
    import os
    from tests.helpers import GOLDEN
    from tests.gpu_util import build_model
    from oracle import params as op
    fx = dict(np.load(os.path.join(GOLDEN, "inverse_mnist.npz")))
    ops, prior_size, M = fo.program("mnist")
    params = op.gen_params(op.param_spec(ops, prior_size, M), int(fx["seed"]))
    for k, v in fx.items():
        if k.startswith("param:"):
            params[k[6:]] = torch.from_numpy(v)
    model = build_model("mnist", params)
    ref = torch.from_numpy(fx["x"])
    for fused in (False, True):                       # per-layer reverse kernels, then the fused inverse steps
        model.fused = fused
        h = model.inverse(torch.from_numpy(fx["z"]).to(DEV))
        # the final floor() makes the output integer valued: only exact-boundary cases may flip by one
        assert (h.cpu() - ref).abs().max() <= 1.0 and (h.cpu() != ref).float().mean() < 2e-3, fused


@pytest.mark.parametrize("B,C,aug,H,W", [(5, 3, 1, 32, 32), (3, 1, 1, 32, 32), (4, 3, 0, 8, 8), (2, 3, 1, 5, 3), (0, 3, 1, 32, 32)])
def test_fused_tail_of_the_inverse_equals_the_layer_chain(L, B, C, aug, H, W):
    """cf_postprocess_inv = [Augment.reverse] -> LogitTransform.reverse -> Normalization.reverse x 2 -> Dequantization.reverse
    (flowsequential.py:32-39 walks them one by one), bitwise: same operations, same order, no fma contraction."""
    from contextflow_amd.layers import _hip
    torch.manual_seed(11)
    z = (torch.randn(B, C + aug, H, W, device=DEV) * 3.0)
    layers = [L.Dequantization(L.UniformDistribution(size=(C, H, W))), L.Normalization(translation=0, scale=256),
              L.Normalization(translation=-1e-6, scale=1 / (1 - 2 * 1e-6)), L.LogitTransform()]
    layers = [m.to(DEV) for m in layers]
    want = z[:, :C] if aug else z
    for m in reversed(layers):
        want = m.reverse(want)
    zz, zbs = _hip.bview(z)
    got = torch.full((B, C, H, W), float("nan"), device=DEV)
    n1, n2 = layers[1], layers[2]
    _hip.call("cf_postprocess_inv", _hip.p(zz), _hip.p(got), B, C * H * W, zbs, n2._t, n2._s, n1._t, n1._s, _hip.stream())
    assert torch.equal(got, want)
    if B:
        assert torch.equal(got, got.floor()) and got.min() >= -1 and got.max() <= 256


def test_inverse_step_tables_follow_the_parameters(L):
    """`inverse` keeps the packed tables of its fused steps (forward fragments of the conditioner, W^-1, inverse ActNorm) between
    calls while their source tensors are unchanged: a second call is bitwise the first; an in-place update of a Conv1x1 weight, of
    an ActNorm shift and of a conditioner weight each changes the result exactly as a fresh packing does; `invalidate_caches()`
    covers writes through `.data`."""
    from tests.gpu_util import build_model
    ops, _, M, params, fx = load_e2e("mnist")
    model = build_model("mnist", params)
    torch.manual_seed(1)
    z = model.dist.sample(9)[0]
    a, b = model.inverse(z), model.inverse(z)
    def inv_slots():
        return [s for s in model.__dict__["_derived"] if s[0] == "inv_ws"]
    assert torch.equal(a, b) and len(inv_slots()) >= 2
    from contextflow_amd.layers import ActNorm, Conv1x1, Coupling
    mods = list(model.sequence_modules)
    conv = next(m for m in mods if isinstance(m, Conv1x1))
    act = next(m for m in mods if isinstance(m, ActNorm))
    cpl = [m for m in mods if isinstance(m, Coupling)][-1]
    with torch.no_grad():
        conv.NN.mul_(1.03)
        act.NN_t.add_(0.05)
        cpl.NN[2].weight.mul_(0.9)
    c = model.inverse(z)                       # the version counters moved: the three steps concerned are packed again
    for s in inv_slots():
        del model.__dict__["_derived"][s]
    d = model.inverse(z)                       # everything packed from scratch
    assert torch.equal(c, d) and not torch.equal(a, c)
    conv.NN.data.mul_(0.5)                     # a write the version counter does not see
    model.invalidate_caches()
    e = model.inverse(z)
    for s in inv_slots():
        del model.__dict__["_derived"][s]
    assert torch.equal(e, model.inverse(z)) and not torch.equal(e, c)


@pytest.mark.parametrize("name", ["mnist", "cifar10"])
def test_sample_shapes_and_prior_consistency(L, name):
    """`sample` runs end to end (SplitPrior.reverse resamples the split halves) and the prior sampler is
    consistent with its own density: E[log p(x)] over samples ~ -entropy bound, finite, and the per-sample
    log_prob returned by `dist.sample` equals `dist.log_prob` of the same draw."""
    from tests.gpu_util import build_model
    ops, _, M, params, fx = load_e2e(name)
    model = build_model(name, params)
    torch.manual_seed(0)
    x = model.sample(6)
    C, H, W = fo.CONFIGS[name][0]
    assert tuple(x.shape) == (6, C, H, W) and torch.isfinite(x).all()
    assert float(x.min()) >= -1.0 and float(x.max()) <= 256.0 and torch.equal(x, x.floor())
    z, lp = model.dist.sample(512)
    assert torch.isfinite(z).all()
    close(model.dist.log_prob(z), lp, tol=1e-6)
    # mixture 1 must explain its own samples better than the other class-mixtures do, on average
    assert int(lp.mean(0).argmax()) == 1


# ------------------------------------------------------------------------------------------ edge cases
@pytest.mark.parametrize("name", ["cifar10", "mnist", "smap"])
def test_edge_batches_and_layouts(L, name):
    """Empty batch, single sample, ragged sizes, non-contiguous and fp64 inputs — fused plan vs the oracle."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e(name)
    model = build_model(name, params)
    C, H, W = fo.CONFIGS[name][0]
    g = torch.Generator().manual_seed(9)
    # empty batch: shape-correct, no launch failures
    set_noise(model, None, [])
    z, logp = model(torch.zeros(0, C, H, W, device=DEV))
    assert tuple(logp.shape) == (0, M) and z.shape[0] == 0
    for B in (1, 3, 17):
        x = torch.rand(B, C, H, W, generator=g) if name == "smap" else torch.randint(0, 256, (B, C, H, W), generator=g).float()
        u = torch.rand(B, C, H, W, generator=g) if name != "smap" else None
        eps = [torch.randn(B, 1, H, W, generator=g)]
        _, ref = fo.flow_forward(ops, params, x, u, eps)
        set_noise(model, u, eps)
        _, logp = model(x.to(DEV))
        assert (bpd(logp.cpu(), name) - bpd(ref, name)).abs().max() < BPD_TOL, B
        # same values through a non-contiguous fp64 view
        xx = x.double().to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not xx.is_contiguous() or B == 1 or C == 1
        set_noise(model, u, eps)
        _, logp2 = model(xx)
        assert (logp2 - logp).abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------ training step (backward)
@pytest.mark.parametrize("name,B,tag", [("mnist", 6, None), ("cifar10", 5, None), ("smap", 7, None), ("atm", 3, None),
                                        ("mnist", 5, "stress"), ("cifar10", 4, "stress"), ("smap", 6, "stress")])
def test_backward_against_autograd_oracle(L, name, B, tag):
    """d sum(w * logp) / d parameters: the hand-written backward (fused HIP step-backward kernel, the layer-by-layer
    backward of TransCoupling / SimpleViT for smap, library GEMMs) against torch.autograd run through the CPU oracle
    in fp64 on the same inputs, noise and parameters."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e(name, tag)           # tag "stress": trained-like parameters (saturated log-scales, ...)
    C, H, W = fo.CONFIGS[name][0]
    g = torch.Generator().manual_seed(21)
    x = torch.rand(B, C, H, W, generator=g) if name in ("smap", "atm") else torch.randint(0, 256, (B, C, H, W), generator=g).float()
    u = torch.rand(B, C, H, W, generator=g)
    eps = [torch.randn(B, 1, H, W, generator=g)]
    if tag:                      # the fixture's own samples: the mixture components sit on THEIR latents (moderate |logp|)
        fxx, fxu, fxe = e2e_inputs(name, fx)
        x, eps = fxx[:B], [e[:B] for e in fxe]
        u = fxu[:B] if fxu is not None else u
    wts = torch.randn(B, M, generator=g)
    # oracle, fp64, autograd
    p64 = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in params.items()}
    _, lp = fo.flow_forward(ops, p64, x.double(), u.double(), [e.double() for e in eps])
    (lp * wts.double()).sum().backward()
    p32 = None
    if tag:                      # stress regime: the fp32 noise floor of the gradients themselves (torch.autograd in fp32)
        p32 = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in params.items()}
        _, lp32 = fo.flow_forward(ops, p32, x, u, eps)
        (lp32 * wts).sum().backward()
    # product
    model = build_model(name, params)
    set_noise(model, u, eps)
    model.train()
    z, logp = model(x.to(DEV))
    assert logp.requires_grad
    (logp * wts.to(DEV)).sum().backward()
    assert (bpd(logp.detach().cpu(), name) - bpd(lp.detach().float(), name)).abs().max() < BPD_TOL
    checked = 0
    for k, p in model.named_parameters():
        ref = p64[k].grad
        if ref is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, k
        got = p.grad.detach().cpu().double()
        scale = max(ref.abs().max().item(), 1e-3)
        err = (got - ref).abs().max().item() / scale
        # measured (tests/dev_bwd_errors.py, profiles/r2_backward_errors.md): worst tensor 4.6e-5 (cifar10 split-prior
        # means), every tensor below the error fp32 torch.autograd itself makes on the same graph (up to 1.8e-4).
        # Stress parameters (sigma down to 0.13, saturated log-scales): the bar is 3x that fp32 floor where it exceeds 1e-4
        tol = 1e-4
        if p32 is not None:
            tol = max(tol, 3.0 * (p32[k].grad.double() - ref).abs().max().item() / scale)
        assert err < tol, "%s: relative grad error %.3e (scale %.3e, bar %.1e)" % (k, err, scale, tol)
        checked += 1
    assert checked >= 30


@pytest.mark.parametrize("name,B", [("mnist", 37), ("cifar10", 70), ("cifar10", 513), ("cifar10", 2049)])   # 513 / 2049: past the row-split / Winograd dispatch thresholds of the 8x8 / 4x4 levels
def test_taped_backward_equals_recompute(L, name, B):
    """Training with the step tape kept (cf_flow_step_fwd_taped writes y0 / h1 / h2 + the aux tape, cf_flow_step_bwd_taped
    reads it) against the form that drops the tape after the forward and rebuilds it per step at backward time
    (TAPE_PLANES = False; also the fallback for batches whose planes would not fit): both run the same taping kernel on the
    same inputs, so logp and every gradient must be BITWISE equal; ragged last tiles at every level."""
    from tests.gpu_util import build_model, set_noise
    from contextflow_amd.layers import flowsequential as fs
    ops, _, M, params, fx = load_e2e(name)
    C, H, W = fo.CONFIGS[name][0]
    g = torch.Generator().manual_seed(33)
    x = torch.randint(0, 256, (B, C, H, W), generator=g).float()
    u = torch.rand(B, C, H, W, generator=g)
    eps = [torch.randn(B, 1, H, W, generator=g)]
    wts = torch.randn(B, M, generator=g).to(DEV)
    out = {}
    try:
        for taped in (True, False):
            fs.TAPE_PLANES = taped
            model = build_model(name, params)
            set_noise(model, u, eps)
            model.train()
            _, logp = model(x.to(DEV))
            (logp * wts).sum().backward()
            out[taped] = (logp.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None})
    finally:
        fs.TAPE_PLANES = True
    assert torch.equal(out[True][0], out[False][0])
    assert out[True][1].keys() == out[False][1].keys() and len(out[True][1]) >= 30
    for k, ga in out[True][1].items():
        assert torch.equal(ga, out[False][1][k]), k


def test_smap_backward_is_additive_over_the_batch(L):
    """Size-independent property of the one-kernel transformer-step backward at a batch the oracle cannot reach: with a loss
    that is a SUM over samples, the gradients of a ragged batch of 5003 (forward in the 8-samples-per-wave form, backward in
    the row-split form, last workgroup three quarters full) equal the sum of the gradients of its two parts (2049 + 2954:
    forward row-split form) - per tensor, to fp32 summation noise - and the input gradient rows are the parts' rows."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e("smap")
    g = torch.Generator().manual_seed(17)
    B, cut = 5003, 2049
    x = torch.rand(B, 25, 8, 1, generator=g)
    eps = torch.randn(B, 1, 8, 1, generator=g)
    wts = torch.randn(B, 1, generator=g).to(DEV)

    def grads(sl):
        model = build_model("smap", params)
        set_noise(model, None, [eps[sl]])
        model.train()
        xin = x[sl].to(DEV).requires_grad_(False)
        _, logp = model(xin)
        (logp * wts[sl]).sum().backward()
        return {k: p.grad.detach().double() for k, p in model.named_parameters() if p.grad is not None}
    whole, a, b = grads(slice(0, B)), grads(slice(0, cut)), grads(slice(cut, B))
    assert whole.keys() == a.keys() == b.keys() and len(whole) >= 500
    worst = 0.0
    for k in whole:
        s = a[k] + b[k]
        scale = max(s.abs().max().item(), 1e-12)
        worst = max(worst, (whole[k] - s).abs().max().item() / scale)
        assert (whole[k] - s).abs().max().item() <= 2e-4 * scale, (k, (whole[k] - s).abs().max().item(), scale)
    print("additivity of the smap backward over 5003 = 2049 + 2954 samples: worst relative difference %.2e" % worst)


@pytest.mark.parametrize("B", [3, 37, 70])
def test_smap_taped_backward_equals_the_recompute_form(L, B):
    """Transformer steps at saturating batches keep the residual stream of the forward (cf_vit_step_fwd with xtape) and the backward
    kernel starts from it (cf_vit_step_bwd with xtape) instead of running the layers again: forced at small, ragged batches
    (the 8-samples-per-wave forward), its gradients equal those of the recompute form to fp32 rounding - the forward's
    residual stream and the row-split kernel's differ by summation order only - and the log-densities are the same bits."""
    import contextflow_amd.layers.flowsequential as fs
    from contextflow_amd.layers.coupling import TransCoupling
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e("smap")
    g = torch.Generator().manual_seed(B)
    x = torch.rand(B, 25, 8, 1, generator=g)
    eps = torch.randn(B, 1, 8, 1, generator=g)
    wts = torch.randn(B, 1, generator=g).to(DEV)

    def run(taped):
        keep, keep_t = TransCoupling.STEP_RS_MAX_BATCH, fs.VSTEP_TAPE
        TransCoupling.STEP_RS_MAX_BATCH, fs.VSTEP_TAPE = 0, taped
        try:
            model = build_model("smap", params)
            set_noise(model, None, [eps])
            model.train()
            _, logp = model(x.to(DEV))
            (logp * wts).sum().backward()
            return logp.detach(), {k: p.grad.detach().double() for k, p in model.named_parameters() if p.grad is not None}
        finally:
            TransCoupling.STEP_RS_MAX_BATCH, fs.VSTEP_TAPE = keep, keep_t
    lp_t, gt_ = run(True)
    lp_r, gr_ = run(False)
    assert torch.equal(lp_t, lp_r)
    # the row-split forward (the default at these batch sizes) tapes the same stream
    model = build_model("smap", params)
    set_noise(model, None, [eps])
    model.train()
    _, logp = model(x.to(DEV))
    (logp * wts).sum().backward()
    for k, p_ in model.named_parameters():
        if p_.grad is not None:
            scale = max(gr_[k].abs().max().item(), 1e-12)
            assert (p_.grad.double() - gr_[k]).abs().max().item() <= 2e-5 * scale, k
    assert gt_.keys() == gr_.keys() and len(gt_) >= 500
    for k in gt_:
        scale = max(gr_[k].abs().max().item(), 1e-12)
        assert torch.isfinite(gt_[k]).all(), k
        assert (gt_[k] - gr_[k]).abs().max().item() <= 2e-5 * scale, (k, (gt_[k] - gr_[k]).abs().max().item(), scale)


@pytest.mark.parametrize("D,H,W,M,K,B", [(8, 16, 16, 10, 5, 7), (16, 8, 8, 10, 5, 9), (64, 4, 4, 10, 5, 6), (8, 7, 7, 3, 2, 5),
                                           (4, 14, 14, 2, 3, 3), (2, 40, 32, 2, 2, 5), (3, 1, 1, 4, 1, 2)])
def test_gmm_ctx_kernels_against_torch(L, D, H, W, M, K, B):
    """cf_gmm_ctx_logprob / cf_gmm_ctx_bwd (several samples per workgroup, channels per wave) against the formula of
    gaussian.py:142-158 in fp64 with torch.autograd: non power-of-two h*w (49, 196), h*w above one register pass
    (1280), a single pixel, batches that leave a ragged last workgroup; with and without the kept log-joints."""
    from contextflow_amd.layers import _hip
    g = torch.Generator().manual_seed(D * 100 + H)
    HW, MK = H * W, M * K
    x = torch.randn(B, D, H, W, generator=g)
    mG, sG = 0.5 * torch.randn(M, K, D, H, W, generator=g), 0.5 * torch.randn(M, K, D, H, W, generator=g) + 0.5
    logw = torch.log_softmax(torch.randn(M, K, generator=g), -1)
    c = 0.3 * torch.randn(B, 2, M, K, D, generator=g)
    gout = torch.randn(B, M, generator=g)
    # fp64 reference
    xr, cr = x.double().requires_grad_(True), c.double().requires_grad_(True)
    mu = mG.double().unsqueeze(0) + cr[:, 0].reshape(B, M, K, D, 1, 1)
    sig = torch.nn.functional.softplus(sG.double().unsqueeze(0) + cr[:, 1].reshape(B, M, K, D, 1, 1))
    lpr = (-0.5 * ((xr.reshape(B, 1, 1, D, H, W) - mu) / sig) ** 2 - torch.log(sig) - 0.5 * math.log(2 * math.pi)).flatten(3).sum(-1) + logw.double()
    ref = torch.logsumexp(lpr, -1)
    (ref * gout.double()).sum().backward()
    d = lambda t: t.contiguous().to(DEV)
    xd, md, sd, ld, cd, gd = d(x), d(mG), d(sG), d(logw), d(c), d(gout)
    out = torch.full((B, M), 2.0, device=DEV)
    lp = torch.empty(B, MK, device=DEV)
    st = _hip.stream()
    _hip.call("cf_gmm_ctx_logprob", _hip.p(xd), _hip.p(md), _hip.p(sd), _hip.p(ld), _hip.p(cd), _hip.p(out), _hip.p(lp),
              B, M, K, D, HW, D * HW, 1, st)
    scale = ref.abs().max().item()
    assert ((out.cpu().double() - 2.0) - ref.detach()).abs().max().item() < 2e-6 * scale + 1e-4
    assert (lp.cpu().double() - lpr.detach().reshape(B, MK)).abs().max().item() < 2e-6 * scale + 1e-4
    for kept in (lp, None):
        gx = torch.full((B, D, H, W), float("nan"), device=DEV)
        gc = torch.full((B, 2 * MK * D), float("nan"), device=DEV)
        _hip.call("cf_gmm_ctx_bwd", _hip.p(xd), _hip.p(md), _hip.p(sd), _hip.p(ld), _hip.p(cd), _hip.p(gd), _hip.p(kept),
                  _hip.p(gx), _hip.p(gc), B, M, K, D, HW, D * HW, st)
        for got, want in ((gx.cpu().double(), xr.grad), (gc.cpu().double().view_as(cr.grad), cr.grad)):
            assert torch.isfinite(got).all()
            assert (got - want).abs().max().item() < 1e-4 * max(want.abs().max().item(), 1e-3)
    # table form: the scale shifts of the batch take U = 3 distinct values, picked by a key per sample
    U = 3
    cs_tab = 0.3 * torch.randn(U, MK, D, generator=g)
    key = torch.randint(0, U, (B,), generator=g)
    c2 = c.clone()
    c2[:, 1] = cs_tab[key].reshape(B, M, K, D)
    c2d, keyd = d(c2), key.to(torch.int32).to(DEV)
    inv, dsg = torch.empty(U, MK * D * HW, device=DEV), torch.empty(U, MK * D * HW, device=DEV)
    lsum = torch.empty(U, MK, device=DEV)
    _hip.call("cf_gmm_ctx_tables", _hip.p(sd), _hip.p(d(cs_tab)), _hip.p(inv), _hip.p(dsg), _hip.p(lsum), U, MK, D, HW, st)
    res = {}
    for tab in (False, True):
        out, lp = torch.zeros(B, M, device=DEV), torch.empty(B, MK, device=DEV)
        gx, gc = torch.full((B, D, H, W), float("nan"), device=DEV), torch.full((B, 2 * MK * D), float("nan"), device=DEV)
        if tab:
            _hip.call("cf_gmm_ctx_logprob_tab", _hip.p(xd), _hip.p(md), _hip.p(inv), _hip.p(lsum), _hip.p(ld), _hip.p(c2d),
                      None, _hip.p(keyd), _hip.p(out), _hip.p(lp), B, M, K, D, HW, D * HW, 0, st)
            # the mean shifts from a table of their own (Um = 2 distinct rows) instead of per-sample rows
            cm_tab = d(c2[:2, 0].reshape(2, MK * D))
            ckey = torch.randint(0, 2, (B,), generator=g)
            c3 = c2.clone()
            c3[:, 0] = c2[:2, 0][ckey]
            o_ref, o_tab = torch.zeros(B, M, device=DEV), torch.zeros(B, M, device=DEV)
            _hip.call("cf_gmm_ctx_logprob_tab", _hip.p(xd), _hip.p(md), _hip.p(inv), _hip.p(lsum), _hip.p(ld), _hip.p(d(c3)),
                      None, _hip.p(keyd), _hip.p(o_ref), None, B, M, K, D, HW, D * HW, 0, st)
            _hip.call("cf_gmm_ctx_logprob_tab", _hip.p(xd), _hip.p(md), _hip.p(inv), _hip.p(lsum), _hip.p(ld), _hip.p(cm_tab),
                      _hip.p(ckey.to(torch.int32).to(DEV)), _hip.p(keyd), _hip.p(o_tab), None, B, M, K, D, HW, D * HW, 0, st)
            assert torch.equal(o_ref, o_tab)
            _hip.call("cf_gmm_ctx_bwd_tab", _hip.p(xd), _hip.p(md), _hip.p(inv), _hip.p(dsg), _hip.p(lsum), _hip.p(ld), _hip.p(c2d),
                      _hip.p(keyd), _hip.p(gd), None, _hip.p(gx), _hip.p(gc), B, M, K, D, HW, D * HW, st)
        else:
            _hip.call("cf_gmm_ctx_logprob", _hip.p(xd), _hip.p(md), _hip.p(sd), _hip.p(ld), _hip.p(c2d), _hip.p(out), _hip.p(lp),
                      B, M, K, D, HW, D * HW, 0, st)
            _hip.call("cf_gmm_ctx_bwd", _hip.p(xd), _hip.p(md), _hip.p(sd), _hip.p(ld), _hip.p(c2d), _hip.p(gd), None, _hip.p(gx),
                      _hip.p(gc), B, M, K, D, HW, D * HW, st)
        res[tab] = (out, lp, gx, gc)
    for a, b_ in zip(res[True], res[False]):
        assert torch.isfinite(a).all()
        assert (a - b_).abs().max().item() < 2e-5 * max(b_.abs().max().item(), 1e-3)


@pytest.mark.parametrize("C,HW,B,cf", [(16, 256, 5, True), (64, 16, 7, False), (76, 72, 3, True), (26, 8, 4, True), (3, 5, 2, False)])
def test_conv1x1_ctx_kernels_against_torch(L, C, HW, B, cf):
    """Per-sample Conv1x1 (conv1x1.py:34-50): W_b = tril(m,-1) + diag(exp(diag m)) [+ NN - I under contextflow],
    z = W_b x, ldj = H W sum diag m - forward and backward (gx, d/dm) against torch.autograd in fp64.  76 channels is
    the ATM specialist (README.md:64-69)."""
    from contextflow_amd.layers import _hip
    g = torch.Generator().manual_seed(C + HW)
    x = torch.randn(B, C, HW, generator=g)
    m = 0.3 * torch.randn(B, C, C, generator=g)
    Wm = torch.linalg.qr(torch.randn(C, C, generator=g))[0].contiguous() if cf else None
    gz, gld = torch.randn(B, C, HW, generator=g), torch.randn(B, generator=g)
    xr, mr = x.double().requires_grad_(True), m.double().requires_grad_(True)
    Wb = torch.tril(mr, -1) + torch.diag_embed(torch.exp(torch.diagonal(mr, dim1=1, dim2=2)))
    if cf:
        Wb = Wb + Wm.double() - torch.eye(C, dtype=torch.float64)
    zr = Wb @ xr
    ldr = HW * torch.diagonal(mr, dim1=1, dim2=2).sum(-1)
    ((zr * gz.double()).sum() + (ldr * gld.double()).sum()).backward()
    d = lambda t: None if t is None else t.contiguous().to(DEV)
    xd, md, Wd, gzd, gldd = d(x), d(m.reshape(B, C * C)), d(Wm), d(gz), d(gld)
    z, ldj = torch.empty(B, C, HW, device=DEV), torch.empty(B, device=DEV)
    st = _hip.stream()
    _hip.call("cf_conv1x1_ctx", _hip.p(xd), _hip.p(md), _hip.p(Wd), _hip.p(z), _hip.p(ldj), B, C, HW, C * HW, st)
    assert (z.cpu().double() - zr.detach()).abs().max().item() < 1e-4 * max(1.0, zr.abs().max().item())
    assert (ldj.cpu().double() - ldr.detach()).abs().max().item() < 1e-4 * max(1.0, ldr.abs().max().item())
    gx, gm = torch.full((B, C, HW), float("nan"), device=DEV), torch.full((B, C * C), float("nan"), device=DEV)
    _hip.call("cf_conv1x1_ctx_bwd", _hip.p(xd), _hip.p(md), _hip.p(Wd), _hip.p(gzd), _hip.p(gldd), _hip.p(gx), _hip.p(gm),
              B, C, HW, C * HW, C * HW, st)
    for got, want in ((gx.cpu().double(), xr.grad), (gm.cpu().double().view(B, C, C), mr.grad)):
        assert torch.isfinite(got).all()
        assert (got - want).abs().max().item() < 1e-4 * max(want.abs().max().item(), 1e-3)


@pytest.mark.parametrize("C", [1, 3, 8, 16, 33, 64, 65, 76, 128, 129, 152, 192])
def test_slogdet_inverse_against_torch(L, C):
    """cf_slogdet_inverse (conv1x1.py:21-31: torch.slogdet / torch.inverse per call): register-resident LU up to 64
    channels, two rows per lane + the LDS Gauss-Jordan inverse up to 128 (ATM: 76), LDS Gauss-Jordan for both up to 192
    (the 144 / 152-wide FC layers of the ATM context-encoder flows) - against torch.linalg in fp64 on
    a perturbed orthogonal matrix with permuted rows (forces pivoting)."""
    from contextflow_amd.layers import _hip
    g = torch.Generator().manual_seed(C)
    q = torch.linalg.qr(torch.randn(C, C, generator=g))[0]
    Wm = ((q + 0.05 * torch.randn(C, C, generator=g)) * (0.5 + torch.rand(C, 1, generator=g)))[torch.randperm(C, generator=g)].contiguous()
    lad, inv = torch.empty(1, device=DEV), torch.full((C, C), float("nan"), device=DEV)
    Wd = Wm.to(DEV)
    _hip.call("cf_slogdet_inverse", _hip.p(Wd), C, _hip.p(lad), _hip.p(inv), _hip.stream())
    ref_l = torch.linalg.slogdet(Wm.double())[1].item()
    ref_i = torch.linalg.inv(Wm.double())
    assert abs(lad.item() - ref_l) < 1e-5 * max(1.0, abs(ref_l))
    assert (inv.cpu().double() - ref_i).abs().max().item() < 2e-5 * ref_i.abs().max().item()
    lad2 = torch.empty(1, device=DEV)
    _hip.call("cf_slogdet_inverse", _hip.p(Wd), C, _hip.p(lad2), None, _hip.stream())       # log|det| alone
    assert abs(lad2.item() - ref_l) < 1e-5 * max(1.0, abs(ref_l))


@pytest.mark.parametrize("tag", ["identity", "leaky", "smooth_leaky", "smooth_tanh", "learnable_leaky", "sigmoid"])
def test_activation_layers_match_reference(L, tag):
    """Identity / LeakyRelu / SmoothLeakyRelu / SmoothTanh / LearnableLeakyRelu / Sigmoid (activations.py:34-118, 213-245)
    through cf_activation: forward, log-det and inverse against the reference classes' outputs (unit_act.npz); a larger
    random tensor round-trips."""
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "unit_act.npz"))
    a, b = (float(v) for v in fx[tag + "/ab"])
    m = {"identity": lambda: L.Identity(), "leaky": lambda: L.LeakyRelu(a), "smooth_leaky": lambda: L.SmoothLeakyRelu(a),
         "smooth_tanh": lambda: L.SmoothTanh(a, b), "learnable_leaky": lambda: L.LearnableLeakyRelu(),
         "sigmoid": lambda: L.Sigmoid(temperature=a, eps=1e-4)}[tag]().to(DEV)
    if tag == "learnable_leaky":
        with torch.no_grad():
            m.alpha_logit.fill_(0.3)
        assert abs(float(m.get_alpha()) - a) < 1e-6
    x = torch.from_numpy(fx[tag + "/x"]).to(DEV)
    z, ldj = m(x)
    assert z.shape == x.shape and tuple(ldj.shape) == tuple(fx[tag + "/ldj"].shape)
    assert (z.cpu() - torch.from_numpy(fx[tag + "/z"])).abs().max() < 2e-6
    assert (ldj.cpu() - torch.from_numpy(fx[tag + "/ldj"])).abs().max() < 2e-4
    assert (m.logdet(x) - ldj).abs().max() == 0
    xr = m.reverse(torch.from_numpy(fx[tag + "/z"]).to(DEV))
    assert (xr.cpu() - torch.from_numpy(fx[tag + "/xr"])).abs().max() < 2e-5
    g = torch.Generator().manual_seed(3)
    big = (3.0 * torch.randn(33, 7, 16, 16, generator=g)).to(DEV) if tag != "sigmoid" else (3.0 * torch.randn(33, 1000, generator=g)).to(DEV)
    zb, lb = m(big)
    assert torch.isfinite(zb).all() and torch.isfinite(lb).all()
    tol = 2e-3 if tag == "sigmoid" else 1e-4                      # sigmoid saturates: the logit of 1 - 1e-4 is the clamp
    sel = (zb > 2e-4) & (zb < 1 - 2e-4) if tag == "sigmoid" else torch.ones_like(zb, dtype=torch.bool)
    assert ((m.reverse(zb) - big).abs()[sel]).max() < tol * max(1.0, big.abs().max().item())
    assert m(torch.zeros(0, 4, 2, 2, device=DEV) if tag != "sigmoid" else torch.zeros(0, 4, device=DEV))[0].shape[0] == 0


def test_gaussian_distribution(L):
    """GaussianDistribution (gaussian.py:75-115): per-channel diagonal Gaussian, log_prob summed over (C, H, W) - against
    torch.distributions in fp64; state_dict keys m / s as upstream."""
    g = torch.Generator().manual_seed(2)
    C, H, W, B = 6, 5, 3, 7
    dist = L.GaussianDistribution((C, H, W)).to(DEV)
    assert set(dist.state_dict()) == {"m", "s"}
    with torch.no_grad():
        dist.m.copy_(torch.randn(C, 1, 1, generator=g))
        dist.s.copy_(torch.randn(C, 1, 1, generator=g))
    x = torch.randn(B, C, H, W, generator=g)
    ref = torch.distributions.Normal(dist.m.cpu().double(), torch.nn.functional.softplus(dist.s.cpu().double())).log_prob(x.double()).sum((1, 2, 3))
    lp = dist.log_prob(x.to(DEV))
    assert tuple(lp.shape) == (B,) and (lp.cpu().double() - ref).abs().max() < 1e-4
    xs, lps = dist.sample(5)
    assert tuple(xs.shape) == (5, C, H, W) and (dist.log_prob(xs) - lps).abs().max() == 0


# ------------------------------------------------------------------------------------------ HIP graph replay
@pytest.mark.parametrize("name", ["mnist", "cifar10"])
def test_graph_capture_matches_eager(L, name):
    """The fused forward captured into a HIP graph replays to the same numbers (fixed noise) on new inputs."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e(name)
    x, u, eps = e2e_inputs(name, fx)
    model = build_model(name, params)
    set_noise(model, u, eps)
    g = model.capture(torch.zeros_like(x).to(DEV))
    _, logp = g(x.to(DEV))
    logp = logp.clone()
    ref = torch.from_numpy(fx["logp"])
    assert (bpd(logp.cpu(), name) - bpd(ref, name)).abs().max() < BPD_TOL
    with torch.no_grad():
        _, eager = model(x.to(DEV))
    assert (logp - eager).abs().max().item() == 0.0
    # second replay, new input: the graph holds pointers to the noise tensors injected at capture time, so those stay
    # in place (replacing them would free memory the graph still reads)
    x2 = torch.roll(x, 1, 0)
    _, lp2 = g(x2.to(DEV))
    with torch.no_grad():
        _, eager2 = model(x2.to(DEV))
    assert (lp2 - eager2).abs().max().item() == 0.0
    assert (lp2 - logp).abs().max().item() > 0.0          # it really is a different result (static buffer was overwritten)


@pytest.mark.parametrize("name", ["mnist", "cifar10"])
def test_captured_train_step_matches_the_eager_loop(L, name):
    """FlowSequential.capture_train_step (forward + loss + hand-written backward + fused AdamW as ONE HIP graph, gradients
    taken from None) against the reference's loop as written (experiment_cl.py:127-136: zero_grad, loss, backward,
    AdamW.step) from the same parameters, inputs and noise: same loss at every step and the same parameters after four
    updates."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e(name)
    x, u, eps = e2e_inputs(name, fx)
    xd = x.to(DEV)
    gt = (torch.arange(x.shape[0]) % M).to(DEV)
    inv = 1.0 / x[0].numel()
    loss_fn = lambda lp, y: torch.nn.functional.cross_entropy(lp * inv, y) if M > 1 else -(lp * inv).mean()
    eager = build_model(name, params)
    set_noise(eager, u, eps)
    eager.train()
    # the same AdamW implementation on both sides: torch's default (for-each) and fused kernels round differently, and four
    # updates at lr = 1e-3 amplify that to 1e-5 of the loss (tools/dev/capture_vs_eager.py: eager + fused == captured exactly)
    opt_e = torch.optim.AdamW(eager.parameters(), lr=1e-3, fused=True, capturable=True)
    losses_e = []
    for _ in range(4):
        opt_e.zero_grad(set_to_none=True)
        loss = loss_fn(eager.log_prob(xd), gt)
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss.detach()))
    cap = build_model(name, params)
    set_noise(cap, u, eps)
    cap.train()
    opt_c = torch.optim.AdamW(cap.parameters(), lr=1e-3, fused=True, capturable=True)
    step = cap.capture_train_step(xd, loss_fn, opt_c)
    l0 = float(step(xd, gt).detach())                      # update 1 (the warm-up step, eager) + capture: returns that step's loss
    assert abs(l0 - losses_e[0]) < 2e-6 * max(1.0, abs(losses_e[0])), (l0, losses_e[0])
    with torch.no_grad():                         # an evaluation between the training steps fills the table caches ...
        cap.log_prob(xd)
    losses_c = [float(step(xd, gt).detach()) for _ in range(3)]           # updates 2-4: replays
    assert step.updates == 4
    for a, b in zip(losses_e[1:], losses_c):
        assert abs(a - b) < 2e-6 * max(1.0, abs(a)), (losses_e, losses_c)
    assert losses_c[-1] < losses_c[0]
    pe, pc = dict(eager.named_parameters()), dict(cap.named_parameters())
    for k in pe:
        d = (pe[k].detach() - pc[k].detach()).abs().max().item()
        assert d < 2e-5 * max(1.0, pe[k].detach().abs().max().item()), (k, d)
    # ... and one after the replays must see the parameters the replays wrote (a graph replay does not move the version
    # counters the caches key on: GraphedTrainStep drops the caches itself)
    fresh = build_model(name, {k: v.detach().cpu() for k, v in cap.state_dict().items()})   # same parameters, no history
    set_noise(fresh, u, eps)
    with torch.no_grad():
        ev_c, ev_f = cap.log_prob(xd), fresh.log_prob(xd)
    assert torch.equal(ev_c, ev_f)
    stale = (bpd(ev_c.cpu(), name) - bpd(torch.from_numpy(fx["logp"]), name)).abs().max()
    assert stale > 1e-3                           # four updates moved the model: a stale cache would reproduce the fixture


def test_auto_graph_replay_and_cache_invalidation(L, monkeypatch):
    """Evaluation under no_grad: the packed parameter tables are cached, and after two identical-shape calls the forward is
    replayed from a captured HIP graph (FlowSequential.auto_graph).  Replays must keep drawing fresh noise, return tensors
    the next call does not overwrite, and a parameter update (version counters) must drop both the graph and the tables."""
    from tests.gpu_util import build_model
    ops, _, M, params, fx = load_e2e("mnist")
    model = build_model("mnist", params)
    from contextflow_amd.layers import graphs
    monkeypatch.setattr(graphs, "_replay_wins", lambda flow, graph, inp: True)  # the mechanics under test; the timing probe has its own test below
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, 256, (48, 1, 32, 32), generator=g).float().to(DEV)
    outs = []
    with torch.no_grad():
        for _ in range(5):
            outs.append(model.log_prob(x))
    st = list(model._graphs.values())
    assert len(st) == 1 and st[0][2] is not None, "no graph captured after repeated identical calls"
    assert len({o.data_ptr() for o in outs}) == 5                       # fresh output tensors
    b = [bpd(o.cpu(), "mnist") for o in outs]
    for i in range(1, 5):
        assert not torch.equal(outs[i], outs[0])                        # fresh dequantisation noise every call / replay
        assert (b[i] - b[0]).abs().max() < 0.4 and abs(float(b[i].mean() - b[0].mean())) < 0.03   # ... of the same distribution
    # a parameter update: results must follow it (stale tables or a stale graph would not)
    with torch.no_grad():
        model.dist.mG.add_(0.5)
        shifted = model.log_prob(x)
        assert list(model._graphs.values())[0][2] is None               # graph dropped, re-armed
        model.auto_graph = False
        ref = model.log_prob(x)
    bs, br = bpd(shifted.cpu(), "mnist"), bpd(ref.cpu(), "mnist")
    assert abs(float(bs.mean() - br.mean())) < 0.03
    assert abs(float(bs.mean() - b[0].mean())) > 0.1                    # the shift is visible


@pytest.mark.parametrize("name,B", [("cifar10", 256), ("cifar10", 37), ("mnist", 64), ("cifar10", 700)])
def test_chained_flow_steps_equal_single_launches(L, name, B):
    """Small batches: the flow steps of a resolution level run as ONE launch (cf_flow_step_fwd_chain: a workgroup owns whole
    samples, steps 2.. run in place on z behind a workgroup barrier).  Bit for bit the log-densities and latents of the same
    plan with one launch per step - at 700 samples only the levels whose small-batch kernels reach that far are chained."""
    from tests.gpu_util import build_model, set_noise
    from contextflow_amd.layers.flowsequential import FlowSequential
    ops, _, M, params, fx = load_e2e(name)
    C, H, W = fo.CONFIGS[name][0]
    g = torch.Generator().manual_seed(B)
    x = torch.randint(0, 256, (B, C, H, W), generator=g).float()
    u, eps = torch.rand(B, C, H, W, generator=g), [torch.randn(B, 1, H, W, generator=g)]
    model = build_model(name, params)
    set_noise(model, u, eps)
    model.auto_graph = False
    launches = []
    orig = _hip_call_counter(launches)
    try:
        with torch.no_grad():
            FlowSequential.CHAIN_STEPS = False
            z0, lp0 = model(x.to(DEV))
            n_single = sum(1 for n in launches if n.startswith("cf_flow_step_fwd"))
            del launches[:]
            FlowSequential.CHAIN_STEPS = True
            z1, lp1 = model(x.to(DEV))
            n_chain = sum(1 for n in launches if n.startswith("cf_flow_step_fwd"))
    finally:
        FlowSequential.CHAIN_STEPS = True
        orig()
    assert torch.equal(lp0, lp1) and torch.equal(z0, z1)
    assert n_chain < n_single, (n_chain, n_single)
    _, ref = fo.flow_forward(ops, params, x[:16], u[:16], [eps[0][:16]])
    assert (bpd(lp1[:16].cpu(), name) - bpd(ref, name)).abs().max() < BPD_TOL


def _hip_call_counter(log):
    """records the entry-point names that go through _hip.call; returns the undo function"""
    from contextflow_amd.layers import _hip
    real = _hip.call

    def counting(name, *a):
        log.append(name)
        return real(name, *a)
    _hip.call = counting
    return lambda: setattr(_hip, "call", real)


def test_replaced_parameter_objects_drop_the_caches(L):
    """A Parameter OBJECT replaced after the caches were filled - `m.NN = nn.Parameter(...)`, `load_state_dict(assign=True)` -
    starts at version 0 again, which would match the version-counter keys of the stale packed tables and captured graphs:
    the process-wide parameter-registration hook (flowsequential._PARAM_GENERATION) makes the flow drop them.  Checked with
    fixed noise (deterministic log-densities): after each replacement the result equals that of a freshly built model with
    the same parameters, and differs from the stale one."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e("mnist")
    x, u, eps = e2e_inputs("mnist", fx)
    model = build_model("mnist", params)
    set_noise(model, u, eps)
    with torch.no_grad():
        base = [model.log_prob(x.to(DEV)) for _ in range(3)][-1]          # caches filled
        conv = next(m for m in model.sequence_modules if isinstance(m, L.Conv1x1))
        conv.NN = torch.nn.Parameter(conv.NN.detach().clone() * 1.25)      # fresh object, version 0, other values
        p2 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        got = model.log_prob(x.to(DEV))
        fresh = build_model("mnist", p2)
        set_noise(fresh, u, eps)
        assert torch.equal(got, fresh.log_prob(x.to(DEV))) and not torch.equal(got, base)
        p3 = {k: (v * 0.5 if k == "dist.mG" else v.clone()) for k, v in p2.items()}
        model.load_state_dict({k: v.to(DEV) for k, v in p3.items()}, assign=True)
        got3 = model.log_prob(x.to(DEV))
        fresh3 = build_model("mnist", p3)
        set_noise(fresh3, u, eps)
        assert torch.equal(got3, fresh3.log_prob(x.to(DEV))) and not torch.equal(got3, got)


def test_user_side_capture_with_a_cold_cache_leaves_no_stale_entries(L):
    """torch.cuda.graph around an evaluation forward whose table cache is cold: the tables are built inside the capture (graph
    pool, captured events) and must NOT be kept as cache entries - the next eager call rebuilds its own and gives the eager
    result."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e("mnist")
    x, u, eps = e2e_inputs("mnist", fx)
    xd = x.to(DEV)
    ref_model = build_model("mnist", params)
    set_noise(ref_model, u, eps)
    model = build_model("mnist", params)
    set_noise(model, u, eps)
    model.auto_graph = False
    with torch.no_grad():
        ref = ref_model.log_prob(xd)
        model._plans[tuple(xd.shape[1:])] = model._build_plan(tuple(xd.shape[1:]))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            torch.zeros(1, device=DEV)                                  # (allocator / lazy-init warm-up on the side stream)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _, captured = model._forward_fused(xd, None)
        assert not model._prep                                          # nothing from inside the capture was cached
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, ref)
        assert torch.equal(model.log_prob(xd), ref)                     # eager call afterwards: own tables, same numbers


def _specialist_eval_model(fxname):
    """(model with every noise source fixed, x, context) of a specialist fixture, on the device."""
    import contextflow_amd as cfa
    from tests.gpu_util import set_noise
    from tests.helpers import load_specialist
    name, ctx, ops, M, params, inp = load_specialist(fxname)
    cfg, ds, MM = cfa.preset_config(name)
    cfg.update(generalist=False, enc_emb=ctx["enc_emb"], enc_type=ctx.get("enc_type", "uniform"), contextflow=ctx["contextflow"])
    model = cfa.create_model(cfg, ds, MM, contexts=ctx["contexts"])
    model.load_state_dict(params, strict=True)
    model = model.to(DEV).eval()
    set_noise(model, inp["u"], inp["eps"])
    encs = [m for m in model.modules() if isinstance(m, cfa.layers.UniformCatDequantization)]
    assert len(encs) == len(inp["cnoise"])
    for e, c in zip(encs, inp["cnoise"]):
        e.fixed_noise = c.to(DEV)
    return model, inp["x"].to(DEV), inp["context"].to(DEV)


def test_parameter_derived_tables_are_built_once_per_parameter_version(L):
    """Every table derived from parameter values (layers/_derived.py, and the `_prep` entries of the fused forward) is built by
    the first call and kept: the second `log_prob`, the second `inverse` and the second specialist evaluation forward launch no
    entry point whose name contains `prepare` and no cf_gmm_ctx_tables.  An in-place update of one Conv1x1 matrix brings the
    prepare launches back for exactly one call, and so does `invalidate_caches()`.  (The bitwise tests cannot see a change that
    quietly stops caching: same numbers, more launches.)"""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e("mnist")
    x, u, eps = e2e_inputs("mnist", fx)
    xd = x.to(DEV)
    model = build_model("mnist", params)
    set_noise(model, u, eps)
    model.auto_graph = False
    spec, xs, cs = _specialist_eval_model("mnist_eye_cf")
    torch.manual_seed(1)
    z = model.dist.sample(9)[0]
    log = []

    def builds(run):
        del log[:]
        run()
        return [n for n in log if "prepare" in n or n == "cf_gmm_ctx_tables"]
    undo = _hip_call_counter(log)
    try:
        with torch.no_grad():
            for run in (lambda: model.log_prob(xd), lambda: model.inverse(z)):
                assert builds(run) and not builds(run)
            first = builds(lambda: spec(xs, cs))
            assert "cf_flow_step_prepare" in first and "cf_gmm_ctx_tables" in first, first
            assert not builds(lambda: spec(xs, cs))
            conv = next(m for m in model.sequence_modules if isinstance(m, L.Conv1x1))
            conv.NN.mul_(1.03)
            for run in (lambda: model.log_prob(xd), lambda: model.inverse(z)):
                assert builds(run) and not builds(run)
            model.invalidate_caches()
            spec.invalidate_caches()
            assert builds(lambda: model.log_prob(xd)) and builds(lambda: model.inverse(z)) and builds(lambda: spec(xs, cs))
    finally:
        undo()


def test_auto_graph_keeps_eager_where_replay_loses(L, monkeypatch):
    """The replay-or-eager decision is measured once per input shape and kept across parameter updates; a shape whose probe
    said "eager" is never captured again, and the probe leaves torch's generator where it was (same noise either way)."""
    from tests.gpu_util import build_model
    ops, _, M, params, fx = load_e2e("mnist")
    x = torch.randint(0, 256, (32, 1, 32, 32), generator=torch.Generator().manual_seed(5)).float().to(DEV)
    from contextflow_amd.layers import graphs
    replay_wins = graphs._replay_wins
    res = {}
    for verdict in (True, False):
        model = build_model("mnist", params)
        probes = []
        monkeypatch.setattr(graphs, "_replay_wins", lambda flow, graph, inp, v=verdict, p=probes: (p.append(1), replay_wins(flow, graph, inp), v)[2])
        torch.manual_seed(11)
        with torch.no_grad():
            outs = [model.log_prob(x).clone() for _ in range(5)]
            model.dist.mG.add_(0.25)                     # parameter update: graph dropped, the decision stays
            outs += [model.log_prob(x).clone() for _ in range(4)]
        assert len(probes) == 1
        st = list(model._graphs.values())[0]
        assert (st[2] is not None) == verdict
        res[verdict] = outs
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)                         # replayed or eager: the same noise stream, the same numbers


def test_training_steps_reduce_the_loss(L):
    """A few AdamW steps with the reference's classification loss (experiment_cl.py:127-133) through the hand-written
    backward: the loss must go down and stay finite (end-to-end use of the gradients, squeeze-folded steps included)."""
    import contextflow_amd as cfa
    torch.manual_seed(0)
    cfg, ds, M = cfa.preset_config("mnist")
    model = cfa.create_model(cfg, ds, M).to(DEV)
    g = torch.Generator().manual_seed(4)
    B = 96
    gt = torch.randint(0, M, (B,), generator=g)
    x = (torch.randint(0, 200, (B, *ds), generator=g).float() + 5.0 * gt.view(B, 1, 1, 1).float()).clamp(0, 255)
    x, gt = x.to(DEV), gt.to(DEV)
    # no separate init call: as in the reference's loop, the first training forward runs the ActNorm data-dependent
    # init itself and still returns a differentiable logp
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3)
    dim_inv = 1.0 / (ds[0] * ds[1] * ds[2])
    losses = []
    for _ in range(12):
        opt.zero_grad(set_to_none=True)
        logp = dim_inv * model.log_prob(x)
        loss = torch.nn.functional.cross_entropy(logp, gt) + 1e-3 * (-torch.nn.functional.logsigmoid(torch.logsumexp(logp, -1))).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0] - 1e-3, losses


@pytest.mark.parametrize("name,data_parallel", [("cifar10", False), ("mnist", False), ("cifar10", True)])
def test_batched_parameter_work_of_a_level_equals_the_per_step_launches(L, name, data_parallel, monkeypatch):
    """At small batches the weight gradients and parameter chains of the steps of a resolution level go out in one set of
    launches (cf_step_wgrads_batch / cf_step_param_grads_batch, blockIdx.z = step) on a side stream, behind the level's last
    backward kernel: the gradients of every parameter equal those of the per-step launches bit for bit - with the
    data-parallel bucket as their destination as well.  Third setting: WGRAD_SIDE_MAX_BATCH = 0, no side streams, every
    step's parameter work launched by itself on the main stream - the path of every batch above 1 024."""
    import contextflow_amd as cfa
    from contextflow_amd.layers import autograd as ag
    cfg, ds, M = cfa.preset_config(name)
    g = torch.Generator().manual_seed(5)
    B = 48
    x = torch.randint(0, 256, (B, *ds), generator=g).float().to(DEV)
    y = torch.randint(0, M, (B,), generator=g).to(DEV)
    inv = 1.0 / x[0].numel()
    got = {}
    for batch in (True, False, "main stream"):
        monkeypatch.setattr(ag, "WGRAD_BATCH", batch is not False)
        if batch == "main stream":
            monkeypatch.setattr(ag, "WGRAD_SIDE_MAX_BATCH", 0)
        torch.manual_seed(0)
        m = cfa.create_model(cfg, ds, M).to(DEV)
        for q in m.sequence_modules:
            if isinstance(q, cfa.layers.Dequantization):
                q.dist.fixed_noise = torch.rand(B, *ds, generator=torch.Generator().manual_seed(9)).to(DEV)
            if isinstance(q, cfa.layers.Augment):
                q.distribution.fixed_noise = torch.randn(B, 1, ds[1], ds[2], generator=torch.Generator().manual_seed(10)).to(DEV)
        with torch.no_grad():
            m(x)
        m.train()
        m.data_parallel = data_parallel
        torch.nn.functional.cross_entropy(m.log_prob(x) * inv, y).backward()
        torch.cuda.synchronize()
        got[batch] = {k: p.grad.clone() for k, p in m.named_parameters()}
    assert len(got[True]) == len(got[False]) == len(got["main stream"]) > 20
    for k, a in got[True].items():
        assert torch.isfinite(a).all(), k
        assert torch.equal(a, got[False][k]), k
        assert torch.equal(a, got["main stream"][k]), k


@pytest.mark.parametrize("wd,maximize", [(1e-2, False), (0.0, False), (0.3, True)])
def test_fused_adamw_equals_torch_adamw(L, wd, maximize):
    """contextflow_amd.optim.FusedAdamW (one cf_adamw_step_batch launch per 72 tensors) against torch.optim.AdamW: the same
    parameters and moments after six updates on 150 tensors of awkward sizes (1 ... 100 003 elements), to fp32 rounding of the
    same formulas; the state_dict has torch's layout and survives a round trip."""
    import contextflow_amd as cfa
    g = torch.Generator().manual_seed(3)
    sizes = [1, 2, 3, 5, 9, 64, 255, 1024, 1025, 4097, 100003] + [int(torch.randint(1, 3000, (1,), generator=g)) for _ in range(139)]
    base = [torch.randn(n, generator=g) for n in sizes]
    grads = [[torch.randn(n, generator=g) * (10.0 ** float(torch.randint(-3, 2, (1,), generator=g))) for n in sizes] for _ in range(6)]
    pa = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    pb = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    kw = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, maximize=maximize)
    oa, ob = torch.optim.AdamW(pa, **kw), cfa.optim.FusedAdamW(pb, **kw)
    for it, gr in enumerate(grads):
        for p, q, gg in zip(pa, pb, gr):
            p.grad = gg.to(DEV)
            q.grad = gg.to(DEV)
        oa.step()
        ob.step()
        if it == 2:                  # save / load in the middle: torch's layout, moments and step count carried over
            sd = ob.state_dict()
            assert set(sd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"} and "_flat" not in sd["param_groups"][0]
            ob2 = cfa.optim.FusedAdamW(pb, **kw)
            ob2.load_state_dict(sd)
            ob = ob2
    for p, q in zip(pa, pb):
        assert torch.isfinite(q).all()
        assert (p - q).abs().max().item() <= 2e-6 * max(1.0, p.abs().max().item())
        sa, sb = oa.state[p], ob.state[q]
        assert (sa["exp_avg"] - sb["exp_avg"]).abs().max().item() <= 1e-6 * max(1e-3, sa["exp_avg"].abs().max().item())
        assert (sa["exp_avg_sq"] - sb["exp_avg_sq"]).abs().max().item() <= 1e-6 * max(1e-6, sa["exp_avg_sq"].abs().max().item())
        assert float(sb["step"]) == 6.0


def test_captured_training_step_with_fused_adamw_equals_the_eager_loop(L):
    """FlowSequential.capture_train_step with FusedAdamW (its update count lives on the device): four replayed steps give the
    parameters of four eager steps, bit for bit."""
    import contextflow_amd as cfa
    cfg, ds, M = cfa.preset_config("mnist")
    g = torch.Generator().manual_seed(8)
    B = 64
    x = torch.randint(0, 256, (B, *ds), generator=g).float().to(DEV)
    y = torch.randint(0, M, (B,), generator=g).to(DEV)
    inv = 1.0 / x[0].numel()
    loss_fn = lambda lp, yy: torch.nn.functional.cross_entropy(lp * inv, yy)
    res = []
    for captured in (False, True):
        torch.manual_seed(0)
        m = cfa.create_model(cfg, ds, M).to(DEV)
        for q in m.sequence_modules:
            if isinstance(q, cfa.layers.Dequantization):
                q.dist.fixed_noise = torch.rand(B, *ds, generator=torch.Generator().manual_seed(9)).to(DEV)
        with torch.no_grad():
            m(x)
        m.train()
        opt = cfa.optim.FusedAdamW(m.parameters(), lr=1e-3)
        if captured:
            step = m.capture_train_step(x, loss_fn, opt, data_parallel=False)
            losses = [float(step(x, y).detach()) for _ in range(4)]
        else:
            losses = []
            for _ in range(4):
                opt.zero_grad(set_to_none=True)
                l = loss_fn(m.log_prob(x), y)
                l.backward()
                opt.step()
                losses.append(float(l.detach()))
        res.append((losses, [p.detach().clone() for p in m.parameters()]))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)
    assert res[0][0][-1] < res[0][0][0]


def test_chained_transformer_steps_equal_single_launches(L, monkeypatch):
    """Evaluation of the SMAP flow at small batches: its eight transformer flow steps in ONE launch (cf_vit_step_fwd_chain:
    a workgroup owns its four samples end to end, steps 2.. in place on z) - z and logp of the per-step launches bit for bit,
    at a ragged batch as well."""
    import contextflow_amd as cfa
    from contextflow_amd.layers.flowsequential import FlowSequential
    cfg, ds, M = cfa.preset_config("smap")
    torch.manual_seed(0)
    m = cfa.create_model(cfg, ds, M).to(DEV).eval()
    m.auto_graph = False
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        m(torch.rand(256, *ds, generator=g).to(DEV))
        for B in (256, 61, 3):
            x = torch.rand(B, *ds, generator=g).to(DEV)
            for q in m.sequence_modules:             # the same noise in both passes
                if isinstance(q, cfa.layers.Dequantization):
                    q.dist.fixed_noise = torch.rand(B, *ds, generator=g).to(DEV)
                if isinstance(q, cfa.layers.Augment):
                    q.distribution.fixed_noise = torch.randn(B, q.aug_size, ds[1], ds[2], generator=g).to(DEV)
            outs = []
            for chain in (True, False):
                monkeypatch.setattr(FlowSequential, "CHAIN_STEPS", chain)
                m.invalidate_caches()
                z, lp = m(x)
                outs.append((z.clone(), lp.clone()))
            assert torch.isfinite(outs[0][1]).all()
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), B


@pytest.mark.parametrize("name,coupling", [("mnist", "maf"), ("smap", "conv"), ("smap", "maf")])
def test_training_with_generic_conv_couplings(L, name, coupling):
    """`--coupling maf` (MaskedCoupling, ar.py) and `--coupling conv` on a time-series topology ((3,1) kernels, model.py:114):
    the conditioners run on the generic conv kernels; their training step goes through conv_backward.  The first grad-mode
    call initialises the ActNorms; gradients of every parameter match torch.autograd through the fp64 oracle on the flow's
    output; a few optimiser steps reduce the loss."""
    import contextflow_amd as cfa
    from oracle import params as op
    torch.manual_seed(1)
    cfg, ds, M = cfa.preset_config(name)
    cfg = dict(cfg, coupling=coupling)
    model = cfa.create_model(cfg, ds, M).to(DEV)
    g = torch.Generator().manual_seed(8)
    B = 24
    x = torch.rand(B, *ds, generator=g) if name == "smap" else torch.randint(0, 256, (B, *ds), generator=g).float()
    x = x.to(DEV)
    gt = torch.randint(0, M, (B,), generator=g).to(DEV)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    dim_inv = 1.0 / (ds[0] * ds[1] * ds[2])
    losses = []
    for it in range(8):
        opt.zero_grad(set_to_none=True)
        logp = dim_inv * model.log_prob(x)
        assert logp.requires_grad
        loss = -logp.mean() if M == 1 else torch.nn.functional.cross_entropy(logp, gt)
        loss.backward()
        if it == 0:
            got = [p for p in model.parameters() if p.grad is not None]
            assert len(got) >= 20 and all(torch.isfinite(p.grad).all() for p in got)
        opt.step()
        losses.append(float(loss))
    assert all(math.isfinite(v) for v in losses), losses
    assert min(losses[1:]) < losses[0], losses


# ---- bits of the weight gradients -------------------------------------------------------------------------------------------
# sha256 over the output bytes of the three tests below, per parameter set, recorded on an MI355X from the library as it was
# BEFORE cf_wgrad.hip got its one launch plan (commit 46e84f8; two processes, equal digests: profiles/wgrad_plan_parity.txt).
# The inputs come from seeded CPU generators and every sum has a fixed order, so the digests hold from run to run.
WGRAD_SHA = {
    "gemm": {
        (16, 32, 32, 9, 5, 0): "95827ca144c97b958f3b58310d3cbc3270a4fbac37df90cb8f472fc49d1f2b2f",
        (16, 16, 16, 9, 3, 0): "b9ec370906ee5771adddfac8514950ad9624a003d8c71b8c4f2b633a553c0dd2",
        (8, 64, 64, 9, 7, 0): "ff6495c4c3df9ab1ddbca10d598ff27f455a21aa9bfd8e61f52686e721da000a",
        (8, 32, 32, 9, 6, 0): "fabe70ef77279efd872f90ea2426ccecff9e7da7e8e68e519dab7877c6ed9306",
        (4, 128, 128, 9, 9, 0): "9372b4e771c5a8ad94a7ca5185cbf128d399a9439ecc3bf5091a8beea8c6e2e4",
        (4, 64, 64, 9, 6, 0): "88bd76ae908af1e8e93f0d6b9f2fb3a39e9abc6b656ff0a088be2085ac152e93",
        (4, 64, 64, 9, 2, 0): "eb5c602b44f782d6f7f059bf222c76dc2cfb0601fa837fefff54c78e782d0d87",
        (16, 16, 32, 1, 4, 0): "fc3f775f244731673e2f3b308457a90b00b66750863405825a7842932a83bb66",
        (8, 64, 16, 1, 5, 0): "3db2485562aec29f377f57991c67a6b5e0ad9de2edea1e52802740c7515c8b1c",
        (4, 128, 32, 1, 7, 0): "c5140f3fbc439eadd9d8b1cabd12c0e4f8ac0e9269c8ce1c4731221ac5735b9a",
        (4, 24, 40, 1, 3, 0): "43a7ac237069c31e44f824e29907f737d5efa478261db53ab4ffa01bc72f237d",
        (4, 128, 128, 9, 70, 0): "0cc22d43077c74ab0b7dbe53b87e774313226e790258fc8e883b1434447a373d",
        (4, 128, 128, 9, 1100, 0): "73cad7edf51d522cb5762f5395deed7e7c923d937ebdaf1a09d09aff556b0ea2",
        (8, 64, 64, 9, 1100, 0): "fbba6c00e96a4005d3b88d3ccacd826bc0cd9be2a3b15ab130cc68367787f296",
        (16, 32, 8, 1, 4, 0): "737cefb5da7502d397676feeec291f229dfdf765cc55dec01c5dbb0fcf8a9b5b",
        (8, 32, 64, 1, 5, 0): "b543686c862c8b020eb0412de3ed2faf01c020c12f370b6d33b849d329f8d390",
        (4, 64, 128, 1, 7, 0): "e79a921c9b350c2bf0927305da8506314531f59109af6304e5ba6d629a6d1bf9",
        (4, 64, 64, 1, 7, 0): "1aa2ddaccf6e51444f170c45f681b337705faf66d7272e8211b7c31a8cc95230",
        (16, 16, 32, 1, 4, 1): "ce31fb58bc66edf789a5139fe8f08f934560c61343574fece13f9c1067b1fd0c",
    },
    "step": {
        (16, 16, 37): "9b195d9469b8b1e7f4c210756dd93ef5222d4fbab858a9dbfb475f8f58174691",
        (32, 8, 300): "ef639963b5b67ed669a707ba516875fe05af6ce99fb5d478ee62200d743256ac",
        (64, 4, 1030): "0437f4c72e935647ffe81d624ee67be508a5634365e5aff30c98c2aac367a956",
        (8, 16, 5): "1ecda57f074111ff8d17989ecbb682fd724f96aab3a64ab19fa1bebfc0cace31",
        (64, 4, 1100): "56a6d9a8313b50ae1450860c8989b5aef081d87e920acb24c45595398a75de05",
        (32, 8, 1100): "6abb58de274177d6726f6d34254cbac52222d387c50c31223b55935ca4762e90",
    },
    "batch": {
        (16, 16, 21): "b8d4ffa33c515e09c7ce21c6ae6603b13ae64a0a4cd3cec26c53c3d753d237ac",
        (32, 8, 130): "cdffdddfcdb781e8b9964796edc2a864329ce1a5837d93845539a628a198668a",
        (64, 4, 257): "5362a68d0ebcb9c8f439d9414cc7f379c3ae8e1a4d84c0ee07a1f38c3dd9eb59",
        (64, 4, 1100): "f359f1090605dab6077fd890a059095b467db469eb0e8660c40c4cc5bb2aa810",
        (32, 8, 1100): "f539460c71d8b73b9ae20fecad9d500cd8b43c58a90550754d9577f419d4d0eb",
    },
}


def _same_bits_as_recorded(test, key, tensors):
    import hashlib
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    print("WGRAD_SHA %s %r %s" % (test, key, h.hexdigest()))
    assert WGRAD_SHA[test].get(key) == h.hexdigest(), (test, key, h.hexdigest())


# (H, MR, NR, taps, B, floats by which Bm is off 16-byte alignment).  What the plan selects (wg_plan in cf_wgrad.hip), beyond the
# first eleven: 3x3 in the Winograd form with a few chunks per split (B = 70), with its split count at the cap of 256 workgroups
# where the direct form's is not (B = 1100 at 4x4 and 8x8); one skinny 1x1 tile (RT, CT) of the training step each: (2, 1) and (2, 4) at NF = 2, (4, 8) and (4, 4) at NF = 1; an unaligned Bm:
# the staged 1x1 kernel in place of the skinny one.  (4, 24, 40): tile (2, 3) is not built - staged as well.
# LEFT OUT: (16, 128, 128, 9, B = 3), the shape that keeps the direct form.  The library the digests were recorded from (46e84f8)
# cannot run it, in either of the two recording processes: that form stages 256 x (33 + 129) floats = 165 888 B of LDS per
# workgroup, more than a CU has, and cf_wgrad returned `launch failed: invalid argument`.  There are no parent bits to pin; the
# library now refuses the shape by name before the launch (weight gradients).  A kernel for it is a change of its own.
WGRAD_GEMM_CASES = [(16, 32, 32, 9, 5, 0), (16, 16, 16, 9, 3, 0), (8, 64, 64, 9, 7, 0), (8, 32, 32, 9, 6, 0),
                    (4, 128, 128, 9, 9, 0), (4, 64, 64, 9, 6, 0), (4, 64, 64, 9, 2, 0), (16, 16, 32, 1, 4, 0),
                    (8, 64, 16, 1, 5, 0), (4, 128, 32, 1, 7, 0), (4, 24, 40, 1, 3, 0),
                    (4, 128, 128, 9, 70, 0), (4, 128, 128, 9, 1100, 0), (8, 64, 64, 9, 1100, 0),
                    (16, 32, 8, 1, 4, 0), (8, 32, 64, 1, 5, 0), (4, 64, 128, 1, 7, 0), (4, 64, 64, 1, 7, 0), (16, 16, 32, 1, 4, 1)]


@pytest.mark.parametrize("H,MR,NR,taps,B,off", WGRAD_GEMM_CASES,
                         ids=["-".join(map(str, c[:5])) + ("-unaligned" if c[5] else "") for c in WGRAD_GEMM_CASES])
def test_wgrad_gemm_against_torch(L, H, MR, NR, taps, B, off):
    """cf_wgrad: gw[t][m][n] = sum_{b,p} A[b][m][p] * Bm[b][n][reflect-shifted p] and gbias[m] = sum A, against the
    weight / bias gradient of torch's conv2d over a reflect-padded input in fp64 (ragged tiles, tail chunks); the bits
    are those of the recorded digests."""
    from contextflow_amd.layers import _hip
    g = torch.Generator().manual_seed(H * 1000 + MR + NR + taps + B)
    A = torch.randn(B, MR, H, H, generator=g)
    Bm = torch.randn(B, NR, H, H, generator=g)
    w = torch.zeros(MR, NR, 3 if taps == 9 else 1, 3 if taps == 9 else 1, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(MR, dtype=torch.float64, requires_grad=True)
    xin = torch.nn.functional.pad(Bm.double(), (1, 1, 1, 1), mode="reflect") if taps == 9 else Bm.double()
    (torch.nn.functional.conv2d(xin, w, bias) * A.double()).sum().backward()
    ref_w = w.grad.permute(2, 3, 0, 1).reshape(taps, MR, NR)
    Ad = A.reshape(B, MR, H * H).to(DEV)
    Bd = torch.empty(B * NR * H * H + off, device=DEV)[off:].view(B, NR, H * H).copy_(Bm.reshape(B, NR, H * H))
    assert _hip.p(Bd).value % 16 == 4 * off
    gw = torch.empty(taps, MR, NR, device=DEV)
    gb = torch.empty(MR, device=DEV)
    ws = torch.empty(_hip.lib().cf_wgrad_ws_bytes(B, MR, NR, H, H, taps), device=DEV, dtype=torch.uint8)
    _hip.call("cf_wgrad", _hip.p(Ad), _hip.p(Bd), _hip.p(gw), _hip.p(gb), _hip.p(ws), B, MR, NR, H, H, taps, _hip.stream())
    scale = ref_w.abs().max().item()
    assert (gw.cpu().double() - ref_w).abs().max().item() < 1e-5 * scale + 1e-4
    assert (gb.cpu().double() - bias.grad).abs().max().item() < 1e-4 * bias.grad.abs().max().item() + 1e-4
    _same_bits_as_recorded("gemm", (H, MR, NR, taps, B, off), [gw, gb])


@pytest.mark.parametrize("H,MR,NR,B", [(16, 32, 32, 300), (16, 20, 24, 7), (8, 64, 64, 777), (8, 48, 40, 5), (4, 128, 128, 2050),
                                         (4, 72, 100, 9), (4, 128, 128, 3)])
def test_wgrad_3x3_winograd_form_equals_the_direct_form(L, H, MR, NR, B):
    """The two implementations of the 3x3 weight gradient - k_wgrad's direct form (nine taps) and its Winograd form
    F(3x3,2x2) - on the same planes: each within 2e-6 of the fp64 result's largest entry, bias sums equal to 1e-6 relative;
    batches that give every workgroup several chunks, ragged row / column tiles, sample counts that leave the last
    4x4 chunk (4 samples) partly empty."""
    import ctypes
    from contextflow_amd.layers import _hip
    lib = _hip.lib()
    fn = lib.cf_wgrad_form
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 7 + [ctypes.c_void_p]
    g = torch.Generator().manual_seed(H * 7 + MR + NR + B)
    A = torch.randn(B, MR, H * H, generator=g).to(DEV)
    Bm = torch.relu(torch.randn(B, NR, H * H, generator=g)).to(DEV)
    pad = torch.nn.functional.pad(Bm.double().view(B, NR, H, H), (1, 1, 1, 1), mode="reflect").unfold(2, H, 1).unfold(3, H, 1)
    ref = torch.einsum("nmyx,nkabyx->abmk", A.double().view(B, MR, H, H), pad).reshape(9, MR, NR)
    refb = A.double().sum((0, 2))
    ws = torch.empty(lib.cf_wgrad_ws_bytes(B, MR, NR, H, H, 9), device=DEV, dtype=torch.uint8)
    out = []
    for form in (0, 1):
        gw = torch.full((9, MR, NR), float("nan"), device=DEV)
        gb = torch.full((MR,), float("nan"), device=DEV)
        _hip.check(fn(_hip.p(A), _hip.p(Bm), _hip.p(gw), _hip.p(gb), _hip.p(ws), B, MR, NR, H, H, 9, form, _hip.stream()), "cf_wgrad_form")
        assert (gw.double() - ref).abs().max().item() < 2e-6 * ref.abs().max().item(), form
        assert (gb.double() - refb).abs().max().item() < 1e-6 * refb.abs().max().item() + 1e-4, form
        out.append(gw)
    assert (out[0] - out[1]).abs().max().item() < 2e-6 * ref.abs().max().item()


@pytest.mark.parametrize("C,H,B", [(16, 16, 37), (32, 8, 300), (64, 4, 1030), (8, 16, 5), (64, 4, 1100), (32, 8, 1100)])
def test_step_wgrads_equals_four_wgrad_calls(L, C, H, B):
    """cf_step_wgrads (four split-K launches + ONE reduce launch) against four cf_wgrad calls on the same planes:
    bitwise equal (same partials, same summation order), and the bits of the recorded digests."""
    from contextflow_amd.layers import _hip
    lib = _hip.lib()
    HID, HALF, HW = 2 * C, C // 2, H * H
    g = torch.Generator().manual_seed(C + H + B)
    r = lambda rows: torch.randn(B, rows, HW, generator=g).to(DEV)
    s_gh, s_gh2, s_gh1, s_gy, t_h2, t_h1, t_y0, xs = r(C), r(HID), r(HID), r(C), r(HID), r(HID), r(HALF), r(C)
    probs = [(s_gh, t_h2, 1), (s_gh2, t_h1, 9), (s_gh1, t_y0, 1), (s_gy, xs, 1)]
    ref = []
    for A, Bm, taps in probs:
        MR, NR = A.shape[1], Bm.shape[1]
        gw, gb = torch.empty(taps, MR, NR, device=DEV), torch.empty(MR, device=DEV)
        ws = torch.empty(lib.cf_wgrad_ws_bytes(B, MR, NR, H, H, taps), device=DEV, dtype=torch.uint8)
        _hip.call("cf_wgrad", _hip.p(A), _hip.p(Bm), _hip.p(gw), _hip.p(gb), _hip.p(ws), B, MR, NR, H, H, taps, _hip.stream())
        ref += [gw, gb]
    out = []
    for A, Bm, taps in probs:
        out += [torch.full((taps, A.shape[1], Bm.shape[1]), float("nan"), device=DEV), torch.full((A.shape[1],), float("nan"), device=DEV)]
    ws = torch.empty(lib.cf_step_wgrads_ws_bytes(B, C, H, H), device=DEV, dtype=torch.uint8)
    P = _hip.p
    _hip.call("cf_step_wgrads", P(s_gh), P(s_gh2), P(s_gh1), P(s_gy), P(t_h2), P(t_h1), P(t_y0), P(xs), *[P(o) for o in out], P(ws),
              B, C, H, H, C * H * H, 0, _hip.stream())
    ref[2] = ref[2].permute(1, 2, 0).contiguous()            # the 3x3 leaves cf_step_wgrads as (2C, 2C, 3, 3)
    for a, b in zip(ref, out):
        assert torch.equal(a.reshape(-1), b.reshape(-1))
    # the step input read in place: the un-squeezed tensor in front of the step's Squeeze((2,2)), as the first half of the
    # channels of a wider tensor (a SplitPrior's view) - same bits as the squeezed dense copy
    from contextflow_amd.layers.squeeze import squeeze_op
    wide = torch.randn(B, C // 2, 2 * H, 2 * H, generator=g).to(DEV)
    view = wide[:, : C // 4]
    xs2 = squeeze_op(view, (2, 2), False).reshape(B, C, HW).contiguous()
    outs = []
    for xsrc, bst, unsq in ((xs2, C * HW, 0), (view, wide.stride(0), 1)):
        o = [torch.full_like(t, float("nan")) for t in out]
        _hip.call("cf_step_wgrads", P(s_gh), P(s_gh2), P(s_gh1), P(s_gy), P(t_h2), P(t_h1), P(t_y0), P(xsrc), *[P(t) for t in o], P(ws),
                  B, C, H, H, bst, unsq, _hip.stream())
        outs.append(o)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][6], out[6])               # (another input: the comparison above is not vacuous)
    _same_bits_as_recorded("step", (C, H, B), out + outs[1])


@pytest.mark.parametrize("C,H,B", [(16, 16, 21), (32, 8, 130), (64, 4, 257), (64, 4, 1100), (32, 8, 1100)])
def test_batched_step_wgrads_equal_the_single_calls(L, C, H, B):
    """cf_step_wgrads_batch / cf_step_param_grads_batch over n = 10 steps (more than one launch's worth of 8; the first and
    the sixth read their input through a Squeeze index map and a wider batch stride, as the first step of a level does):
    every output bitwise equal to the per-step entry points."""
    import ctypes
    from contextflow_amd.layers import _hip
    lib, P, A = _hip.lib(), _hip.p, _hip.ptr_array
    HID, HALF, HW, n = 2 * C, C // 2, H * H, 10
    g = torch.Generator().manual_seed(C + B)
    r = lambda *sh: torch.randn(*sh, generator=g).to(DEV)
    steps = []
    for i in range(n):
        planes = [r(B, rows, HW) for rows in (C, HID, HID, C, HID, HID, HALF)]
        if i % 5 == 0:
            wide = r(B, C // 2, 2 * H, 2 * H)
            xs, bst, unsq = wide[:, : C // 4], wide.stride(0), 1
        else:
            xs, bst, unsq = r(B, C, HW), C * HW, 0
        steps.append((planes, xs, bst, unsq, wide if i % 5 == 0 else None))
    shapes = [(1, C, HID), (C,), (HID, HID, 3, 3), (HID,), (1, HID, HALF), (HID,), (1, C, C), (C,)]
    wsb = lib.cf_step_wgrads_ws_bytes(B, C, H, H)
    single, batched = [], []
    for planes, xs, bst, unsq, _ in steps:
        o = [torch.full(sh, float("nan"), device=DEV) for sh in shapes]
        ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
        _hip.call("cf_step_wgrads", *[P(t) for t in planes], P(xs), *[P(t) for t in o], P(ws), B, C, H, H, bst, unsq, _hip.stream())
        single.append(o)
        batched.append([torch.full(sh, float("nan"), device=DEV) for sh in shapes])
    wss = [torch.empty(wsb, device=DEV, dtype=torch.uint8) for _ in range(n)]
    bst_arr = (ctypes.c_int64 * n)(*[st[2] for st in steps])
    sq_arr = (ctypes.c_int * n)(*[st[3] for st in steps])
    _hip.call("cf_step_wgrads_batch", n, *[A([st[0][k] for st in steps]) for k in range(7)], A([st[1] for st in steps]),
              *[A([o[k] for o in batched]) for k in range(8)], A(wss), B, C, H, H, ctypes.cast(bst_arr, ctypes.c_void_p),
              ctypes.cast(sq_arr, ctypes.c_void_p), _hip.stream())
    for i in range(n):
        for a, b in zip(single[i], batched[i]):
            assert torch.isfinite(a).all() and torch.equal(a, b), i
    _same_bits_as_recorded("batch", (C, H, B), [t for o in batched for t in o])
    # the parameter chains behind them
    Wm = [torch.linalg.qr(torch.randn(C, C, generator=g))[0].contiguous().to(DEV) for _ in range(n)]
    t, logs, winv = [0.1 * r(C) for _ in range(n)], [0.1 * r(C) for _ in range(n)], [r(C, C) for _ in range(n)]
    gsum = r(1)
    outs = {}
    for mode in ("single", "batch"):
        gNN, gt, gl = ([torch.full((C, C), float("nan"), device=DEV) for _ in range(n)], [torch.full((C,), float("nan"), device=DEV) for _ in range(n)],
                       [torch.full((C,), float("nan"), device=DEV) for _ in range(n)])
        gWp = [o[6][0].contiguous() for o in single]
        gbp = [o[7] for o in single]
        if mode == "single":
            for i in range(n):
                _hip.call("cf_step_param_grads", P(gWp[i]), P(gbp[i]), P(Wm[i]), P(t[i]), P(logs[i]), P(winv[i]), P(gsum), HW, P(gNN[i]), P(gt[i]),
                          P(gl[i]), C, _hip.stream())
        else:
            _hip.call("cf_step_param_grads_batch", n, A(gWp), A(gbp), A(Wm), A(t), A(logs), A(winv), P(gsum), HW, A(gNN), A(gt), A(gl), C,
                      _hip.stream())
        outs[mode] = gNN + gt + gl
    for a, b in zip(outs["single"], outs["batch"]):
        assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("C,H,B", [(16, 16, 5), (32, 8, 37), (64, 4, 300), (64, 4, 1), (64, 4, 3), (64, 4, 1700), (8, 16, 3)])
def test_step_backward_writes_the_unsqueezed_gradient(L, C, H, B):
    """cf_flow_step_bwd_taped with gx_unsqueezed: dL/dx in the layout of the tensor in front of the step's Squeeze((2,2)) =
    squeeze_op(inverse) of the squeezed-layout result, bit for bit (ragged last workgroup included)."""
    from contextflow_amd.layers import _hip
    from contextflow_amd.layers.squeeze import squeeze_op
    from contextflow_amd.layers.flowsequential import step_tape
    lib = _hip.lib()
    g = torch.Generator().manual_seed(C * 7 + B)
    HID, HALF, HW = 2 * C, C // 2, H * H
    r = lambda *sh: torch.randn(*sh, generator=g).to(DEV)
    Wm = torch.linalg.qr(torch.randn(C, C, generator=g))[0].contiguous().to(DEV)
    t, logs = 0.1 * r(C), 0.1 * r(C)
    w1, b1, w2, b2, w3, b3 = 0.2 * r(HID, HALF, 1, 1), 0.1 * r(HID), 0.05 * r(HID, HID, 3, 3), 0.1 * r(HID), 0.05 * r(C, HID, 1, 1), 0.1 * r(C)
    P, st = _hip.p, _hip.stream()
    ws = torch.empty(lib.cf_flow_step_ws_bytes(C, H, H), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_prepare", P(Wm), P(t), P(logs), P(w1), P(b1), P(w2), P(b2), P(w3), P(b3), P(ws), C, H, H, st)
    wsb = torch.empty(lib.cf_flow_step_bwd_ws_bytes(C, H, H), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_bwd_prepare", P(Wm), P(logs), P(w1), P(w2), P(w3), P(wsb), C, H, H, st)
    x = r(B, C, H, H)
    z, ld = torch.empty_like(x), torch.zeros(B, device=DEV)
    planes = step_tape(B, C, H, H, DEV)
    _hip.call("cf_flow_step_fwd_taped", P(x), P(z), P(ld), P(ws), P(planes[0]), P(planes[1]), P(planes[2]), P(planes[3]), B, C, H, H,
              C * HW, 0, st)
    gz, gld = r(B, C, H, H), r(B)
    res = []
    for unsq in (0, 1):
        gx = torch.full((B, C, H, H), float("nan"), device=DEV)
        pl = [torch.empty(B, rows, HW, device=DEV) for rows in (C, HID, HID, C)]
        _hip.call("cf_flow_step_bwd_taped", P(gz), P(gld), P(wsb), P(planes[3]), P(gx), *[P(p_) for p_ in pl], B, C, H, H, unsq, st)
        res.append(gx)
    want = squeeze_op(res[0], (2, 2), True)
    assert torch.isfinite(res[1]).all()
    assert torch.equal(res[1].view_as(want), want)


def test_one_sample_backward_of_the_4x4_level_equals_the_tile_form(L):
    """cf_flow_step_bwd_taped at the 4x4 level runs one sample per workgroup (k_flow_step_bwd_rs16: 16x16x4 tiles, natural
    row order, adjoint of the reflect gather on the operand; its tape comes from the one-sample forward k_flow_step_rs16) up
    to 1536 samples and the 8-samples-per-workgroup kernel above: the same samples through both (a batch of 512, and the
    first 512 of a batch of 1600 - tape from the tile-form forward) agree to the rounding of two accumulation orders in
    dL/dx and in all four weight-gradient operand planes, for both layouts of dL/dx."""
    from contextflow_amd.layers import _hip
    from contextflow_amd.layers.flowsequential import step_tape
    lib = _hip.lib()
    C, H = 64, 4
    g = torch.Generator().manual_seed(41)
    HID, HALF, HW = 2 * C, C // 2, H * H
    r = lambda *sh: torch.randn(*sh, generator=g).to(DEV)
    Wm = torch.linalg.qr(torch.randn(C, C, generator=g))[0].contiguous().to(DEV)
    t, logs = 0.1 * r(C), 0.1 * r(C)
    w1, b1, w2, b2, w3, b3 = 0.2 * r(HID, HALF, 1, 1), 0.1 * r(HID), 0.05 * r(HID, HID, 3, 3), 0.1 * r(HID), 0.05 * r(C, HID, 1, 1), 0.1 * r(C)
    P, st = _hip.p, _hip.stream()
    ws = torch.empty(lib.cf_flow_step_ws_bytes(C, H, H), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_prepare", P(Wm), P(t), P(logs), P(w1), P(b1), P(w2), P(b2), P(w3), P(b3), P(ws), C, H, H, st)
    wsb = torch.empty(lib.cf_flow_step_bwd_ws_bytes(C, H, H), device=DEV, dtype=torch.uint8)
    _hip.call("cf_flow_step_bwd_prepare", P(Wm), P(logs), P(w1), P(w2), P(w3), P(wsb), C, H, H, st)
    xa, gza, glda = r(1600, C, H, H), r(1600, C, H, H), r(1600)

    def run(B, unsq):
        x, gz, gld = xa[:B].contiguous(), gza[:B].contiguous(), glda[:B].contiguous()
        z, ld = torch.empty_like(x), torch.zeros(B, device=DEV)
        planes = step_tape(B, C, H, H, DEV)
        _hip.call("cf_flow_step_fwd_taped", P(x), P(z), P(ld), P(ws), P(planes[0]), P(planes[1]), P(planes[2]), P(planes[3]), B, C, H, H,
                  C * HW, 0, st)
        gx = torch.full((B, C, H, H), float("nan"), device=DEV)
        pl = [torch.full((B, rows, HW), float("nan"), device=DEV) for rows in (C, HID, HID, C)]
        _hip.call("cf_flow_step_bwd_taped", P(gz), P(gld), P(wsb), P(planes[3]), P(gx), *[P(p_) for p_ in pl], B, C, H, H, unsq, st)
        return [gx] + pl

    for unsq in (0, 1):
        one, tile = run(512, unsq), run(1600, unsq)
        for name, a, b in zip(("gx", "g_h", "g_h2", "g_h1", "g_y"), one, tile):
            assert torch.isfinite(a).all(), name
            err = (a.double() - b[:512].double()).abs().max().item()
            assert err <= 2e-6 * b.abs().max().item(), (name, unsq, err)
        # the ReLU masks are the tape's in both forms: exact zeros at the same places
        assert torch.equal(one[2] == 0, tile[2][:512] == 0) and torch.equal(one[3] == 0, tile[3][:512] == 0)


@pytest.mark.parametrize("C,H", [(16, 16), (32, 8), (64, 4)])
def test_prepare_train_equals_prepare_plus_inverse(L, C, H):
    """cf_flow_step_prepare_train: the packed tables are bitwise those of cf_flow_step_prepare, and the W^-1 it writes from
    the same factorisation is the inverse (against fp64 torch; what d log|det W| / dW = W^-T needs)."""
    from contextflow_amd.layers import _hip
    lib, P = _hip.lib(), _hip.p
    g = torch.Generator().manual_seed(C)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.2).to(DEV)
    HID, HALF = 2 * C, C // 2
    Wm = (torch.linalg.qr(torch.randn(C, C, generator=g))[0] + 0.05 * torch.randn(C, C, generator=g)).contiguous().to(DEV)
    args = [Wm, r(C), r(C), r(HID, HALF), r(HID), r(HID, HID, 3, 3), r(HID), r(C, HID), r(C)]
    n = lib.cf_flow_step_ws_bytes(C, H, H)
    ws0 = torch.zeros(n, device=DEV, dtype=torch.uint8)
    ws1 = torch.zeros(n, device=DEV, dtype=torch.uint8)
    winv = torch.empty(C, C, device=DEV)
    _hip.call("cf_flow_step_prepare", *[P(a) for a in args], P(ws0), C, H, H, _hip.stream())
    _hip.call("cf_flow_step_prepare_train", *[P(a) for a in args], P(ws1), P(winv), C, H, H, _hip.stream())
    assert torch.equal(ws0, ws1)
    ref = torch.linalg.inv(Wm.double().cpu())
    assert (winv.double().cpu() - ref).abs().max().item() < 1e-5 * ref.abs().max().item()


@pytest.mark.parametrize("rows,K,N", [(1000, 104, 52), (37, 52, 104), (513, 64, 192), (300, 30, 17), (128, 152, 152)])
def test_linear_tn_equals_linear_with_a_transposed_copy(L, rows, K, N):
    """cf_linear_tn (gx = gy W, the nn.Linear weight as stored) against cf_linear on W^T copied out: bitwise equal (same
    LDS image, same summation order), ragged row / feature tiles, K not a multiple of 4."""
    from contextflow_amd.layers import _hip
    g = torch.Generator().manual_seed(rows + K + N)
    gy = torch.randn(rows, K, generator=g).to(DEV)
    W = torch.randn(K, N, generator=g).to(DEV)                # the layer's (out = K here, in = N) weight
    a, b = torch.empty(rows, N, device=DEV), torch.empty(rows, N, device=DEV)
    _hip.call("cf_linear", _hip.p(gy), _hip.p(W.t().contiguous()), None, None, _hip.p(a), rows, K, N, 0, _hip.stream())
    _hip.call("cf_linear_tn", _hip.p(gy), _hip.p(W), _hip.p(b), rows, K, N, _hip.stream())
    assert torch.equal(a, b)
    ref = gy.double() @ W.double()
    assert (b.double() - ref).abs().max().item() < 1e-5 * ref.abs().max().item()


def test_layer_backward_kernels_against_torch(L):
    """cf_layernorm_bwd / cf_attention_bwd / cf_gelu / cf_coupling_apply_bwd / cf_channel_sums against torch.autograd
    in fp64 (ragged row counts, the SMAP ViT geometry: dim 52, 4 tokens, head 64)."""
    from contextflow_amd.layers import _hip
    g = torch.Generator().manual_seed(5)
    st = _hip.stream
    keep = []

    def P(t):                                # device copies must outlive the (asynchronous) kernel launch
        if t is None:
            return None
        t = t.to(DEV).contiguous()
        keep.append(t)
        return _hip.p(t)
    # LayerNorm (dim 152 = the ATM transformer width)
    for rows, dim in ((4 * 37 + 3, 52), (36 * 5 + 1, 152), (7, 256)):
        x = torch.randn(rows, dim, generator=g); w = torch.randn(dim, generator=g); b = torch.randn(dim, generator=g); gy = torch.randn(rows, dim, generator=g)
        x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
        torch.nn.functional.layer_norm(x64, (dim,), w64, b64, 1e-5).backward(gy.double())
        gx = torch.empty(rows, dim, device=DEV); nparts = _hip.lib().cf_layernorm_bwd_parts()
        part = torch.empty(nparts, 2 * dim, device=DEV)
        _hip.call("cf_layernorm_bwd", P(x.cpu()), P(w.cpu()), P(gy.cpu()), _hip.p(gx), _hip.p(part), rows, dim, 1e-5, st())
        s = part.sum(0).cpu().double()
        assert (gx.cpu().double() - x64.grad).abs().max() < 1e-4
        assert (s[:dim] - w64.grad).abs().max() < 1e-3 and (s[dim:] - b64.grad).abs().max() < 1e-3
    # attention, forward and backward (4 tokens: SMAP; 36 / 9: ATM levels)
    for B, N, dh in ((9, 4, 64), (5, 36, 64), (3, 9, 64), (2, 17, 32)):
        qkv = torch.randn(B * N, 3 * dh, generator=g); go = torch.randn(B * N, dh, generator=g)
        q64 = qkv.double().requires_grad_(True)
        q, k, v = q64.view(B, N, 3 * dh).split(dh, dim=-1)
        out = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, dim=-1) @ v
        out.backward(go.double().view(B, N, dh))
        of = torch.empty(B * N, dh, device=DEV)
        _hip.call("cf_attention", P(qkv.cpu()), _hip.p(of), B, N, dh, dh ** -0.5, st())
        assert (of.cpu().double() - out.detach().reshape(B * N, dh)).abs().max() < 1e-5
        gq = torch.empty(B * N, 3 * dh, device=DEV)
        _hip.call("cf_attention_bwd", P(qkv.cpu()), P(go.cpu()), _hip.p(gq), B, N, dh, dh ** -0.5, st())
        assert (gq.cpu().double() - q64.grad).abs().max() < 1e-4
    # linear: K walked in chunks of 32 (ragged last chunk, odd K), ragged rows / features, bias, residual, activations
    for rows, K, N, act, use_res in ((300, 152, 152, 0, True), (129, 7, 200, 2, False), (64, 33, 5, 1, False), (1000, 256, 96, 0, False),
                                     (37, 128, 97, 1, True)):
        xl = torch.randn(rows, K, generator=g); wl = torch.randn(N, K, generator=g) / K ** 0.5; bl = torch.randn(N, generator=g)
        rl = torch.randn(rows, N, generator=g) if use_res else None
        ref = xl.double() @ wl.double().t() + bl.double()
        ref = torch.nn.functional.gelu(ref) if act == 1 else (torch.relu(ref) if act == 2 else ref)
        if use_res:
            ref = ref + rl.double()
        yl = torch.full((rows, N), float("nan"), device=DEV)
        _hip.call("cf_linear", P(xl), P(wl), P(bl), P(rl) if use_res else None, _hip.p(yl), rows, K, N, act, st())
        assert (yl.cpu().double() - ref).abs().max() < 2e-5 * max(1.0, ref.abs().max().item()), (rows, K, N, act)
    # weight / bias gradient of a Linear: split-K over the rows (ragged last chunk, > 256 chunks, several tile blocks)
    # wide problems run as column blocks (<= 128 outputs x <= 255 inputs): the mixture backward's (80 x B)(B x 1024) sums,
    # 300 x 300, more than 128 outputs with more than 255 inputs
    for rows, K, N in ((300, 152, 152), (36 * 300 + 5, 152, 192), (129, 7, 200), (64, 33, 5), (2000, 150, 200), (5, 64, 64),
                       (700, 1024, 80), (8, 300, 300), (333, 513, 130)):
        xl = torch.randn(rows, K, generator=g); gl = torch.randn(rows, N, generator=g)
        gW, gb = torch.full((N, K), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
        wsb = torch.empty(_hip.lib().cf_linear_wgrad_ws_bytes(rows, K, N), device=DEV, dtype=torch.uint8)
        _hip.call("cf_linear_wgrad", P(xl), P(gl), _hip.p(gW), _hip.p(gb), _hip.p(wsb), rows, K, N, st())
        rW, rb = gl.double().t() @ xl.double(), gl.double().sum(0)
        assert (gW.cpu().double() - rW).abs().max() < 2e-5 * max(1.0, rW.abs().max().item()), (rows, K, N)
        assert (gb.cpu().double() - rb).abs().max() < 2e-5 * max(1.0, rb.abs().max().item()), (rows, K, N)
        if K >= 300:                                      # x squared while staged (second-moment sums)
            g2 = torch.full((N, K), float("nan"), device=DEV)
            _hip.call("cf_linear_wgrad_x2", P(xl), P(gl), _hip.p(g2), _hip.p(wsb), rows, K, N, st())
            r2 = gl.double().t() @ (xl.double() ** 2)
            assert (g2.cpu().double() - r2).abs().max() < 2e-5 * max(1.0, r2.abs().max().item()), (rows, K, N)
    # GELU
    xg = torch.randn(1000, generator=g) * 2; gg = torch.randn(1000, generator=g)
    x64 = xg.double().requires_grad_(True)
    y64 = torch.nn.functional.gelu(x64); y64.backward(gg.double())
    yo = torch.empty(1000, device=DEV); go2 = torch.empty(1000, device=DEV)
    _hip.call("cf_gelu", P(xg.cpu()), None, _hip.p(yo), 1000, 0, st())
    _hip.call("cf_gelu", P(xg.cpu()), P(gg.cpu()), _hip.p(go2), 1000, 1, st())
    assert (yo.cpu().double() - y64.detach()).abs().max() < 1e-6 and (go2.cpu().double() - x64.grad).abs().max() < 1e-5
    # affine coupling map
    B, C, HW = 5, 26, 8
    xc = torch.randn(B, C, HW, generator=g); h = torch.randn(B, C, HW, generator=g); gz = torch.randn(B, C, HW, generator=g); gl = torch.randn(B, generator=g)
    x64, h64 = xc.double().requires_grad_(True), h.double().requires_grad_(True)
    ls = 2 * torch.tanh(h64[:, C // 2:] / 2)
    z = torch.cat([x64[:, :C // 2], x64[:, C // 2:] * torch.exp(ls) + h64[:, :C // 2]], 1)
    ((z * gz.double()).sum() + (ls.flatten(1).sum(-1) * gl.double()).sum()).backward()
    gxo, gho = torch.empty(B, C, HW, device=DEV), torch.empty(B, C, HW, device=DEV)
    _hip.call("cf_coupling_apply_bwd", P(xc.cpu()), P(h.cpu()), P(gz.cpu()), P(gl.cpu()), _hip.p(gxo), _hip.p(gho), B, C, HW, C * HW, C * HW, st())
    assert (gxo.cpu().double() - x64.grad).abs().max() < 1e-5 and (gho.cpu().double() - h64.grad).abs().max() < 1e-5
    # channel sums
    a, b2 = torch.randn(B, C, HW, generator=g), torch.randn(B, C, HW, generator=g)
    out = torch.empty(2 * C, device=DEV)
    wsum = torch.empty(_hip.lib().cf_channel_sums_ws_bytes(B, C), device=DEV, dtype=torch.uint8)
    _hip.call("cf_channel_sums", P(a.cpu()), P(b2.cpu()), _hip.p(out), _hip.p(wsum), B, C, HW, C * HW, C * HW, st())
    assert (out[:C].cpu() - a.sum((0, 2))).abs().max() < 1e-4 and (out[C:].cpu() - (a * b2).sum((0, 2))).abs().max() < 1e-4
    Bb = 1000                                                 # more samples than batch slices: ragged slices
    a, b2 = torch.randn(Bb, C, HW, generator=g), torch.randn(Bb, C, HW, generator=g)
    wsum = torch.empty(_hip.lib().cf_channel_sums_ws_bytes(Bb, C), device=DEV, dtype=torch.uint8)
    _hip.call("cf_channel_sums", P(a.cpu()), P(b2.cpu()), _hip.p(out), _hip.p(wsum), Bb, C, HW, C * HW, C * HW, st())
    assert (out[:C].cpu() - a.sum((0, 2))).abs().max() < 1e-3 and (out[C:].cpu() - (a * b2).sum((0, 2))).abs().max() < 1e-3


def test_training_steps_reduce_the_loss_smap(L):
    """AdamW steps on the SMAP transformer flow with the reference's anomaly-detection loss (experiment_ad.py:204-210:
    negative mean log-likelihood per dimension) through the layer-by-layer backward: the loss must go down."""
    import contextflow_amd as cfa
    torch.manual_seed(0)
    cfg, ds, M = cfa.preset_config("smap")
    model = cfa.create_model(cfg, ds, M).to(DEV)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(128, *ds, generator=g).to(DEV)
    with torch.no_grad():
        model(x)                                         # ActNorm data-dependent init
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    dim_inv = 1.0 / (ds[0] * ds[1] * ds[2])
    losses = []
    for _ in range(8):
        opt.zero_grad(set_to_none=True)
        loss = -(dim_inv * model.log_prob(x)).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0] - 1e-3, losses


# ------------------------------------------------------------------------------------------ specialist (context) mode
@pytest.mark.parametrize("fxname", ["mnist_eye_cf", "mnist_onehot", "cifar10_onehot_cf", "cifar10_eye",
                                    "cifar10_onehot_vardeq", "cifar10_eye_vardeq_cf", "smap_onehot_cf", "smap_eye",
                                    "cifar10_eye_argmax_cf", "cifar10_embed_eyesample", "mnist_embed_probsample_cf",
                                    "atm_onehot_cf", "atm_embed_eyesample_cf", "atm_onehot_vardeq_cf", "atm_eye_argmax_cf",
                                    "atm_embed_probsample_cf"])
def test_specialist_forward_matches_reference(L, fxname):
    """Context-conditioned models (create_model(generalist=False), model.py:117-162): per-sample Conv1x1 / ActNorm /
    Coupling parameters from the context encoders + CN nets, context-shifted GMM priors — logp against the reference's
    own output on the captured noise (tests/golden/spec_*.npz)."""
    import contextflow_amd as cfa
    from tests.helpers import load_specialist
    name, ctx, ops, M, params, inp = load_specialist(fxname)
    cfg, ds, MM = cfa.preset_config(name)
    enc_type = ctx.get("enc_type", "uniform")
    cfg.update(generalist=False, enc_emb=ctx["enc_emb"], enc_type=enc_type, contextflow=ctx["contextflow"])
    model = cfa.create_model(cfg, ds, MM, contexts=ctx["contexts"])
    model.load_state_dict(params, strict=True)
    model = model.to(DEV).eval()
    from tests.gpu_util import set_noise
    set_noise(model, inp["u"], inp["eps"])
    noisy = cfa.layers.UniformCatDequantization if enc_type == "uniform" else cfa.layers.ConditionalGaussianDistribution
    encs = [m for m in model.modules() if isinstance(m, noisy)]
    assert len(encs) == len(inp["cnoise"])
    for e, c in zip(encs, inp["cnoise"]):
        e.fixed_noise = c.to(DEV)
    z, logp = model(inp["x"].to(DEV), inp["context"].to(DEV))
    # |logp| reaches 1.4e5 in the vardeq fixture: one fp32 ulp there is 0.0156 nats = 7e-6 bits/dim, and the reference
    # itself differs from its own fp64 evaluation by that much (make_golden_specialist.py prints 7.6e-6)
    tol = 3e-5 if fxname == "cifar10_onehot_vardeq" else BPD_TOL
    tol = max(tol, 1e-5 * bpd(inp["logp"], name).abs().max().item())    # un-normalised smap_eye: |logp| ~ 1e6
    assert (bpd(logp.cpu(), name) - bpd(inp["logp"], name)).abs().max().item() < tol
    assert (z.cpu() - inp["z"]).abs().max().item() < 2e-3 * max(1.0, inp["z"].abs().max().item())
    # ragged batch / different contexts per sample: first two samples alone give the same rows
    for e, c in zip(encs, inp["cnoise"]):
        e.fixed_noise = c[:2].to(DEV)
    set_noise(model, inp["u"][:2], [e[:2] for e in inp["eps"]])
    _, logp2 = model(inp["x"][:2].to(DEV), inp["context"][:2].to(DEV))
    assert (logp2 - logp[:2]).abs().max().item() < 2e-2 * max(1.0, 1e-5 * logp.abs().max().item())


@pytest.mark.parametrize("fxname", ["mnist_eye_cf", "cifar10_onehot_cf", "smap_onehot_cf", "atm_onehot_cf", "atm_embed_eyesample_cf",
                                    "mnist_onehot", "cifar10_eye", "cifar10_embed_eyesample", "cifar10_eye_vardeq_cf",
                                    "cifar10_eye_argmax_cf", "mnist_embed_probsample_cf", "cifar10_onehot_vardeq", "smap_eye"])
def test_specialist_backward_against_autograd_oracle(L, fxname):
    """Specialist training: d sum(w * logp) / d parameters from the hand-written backward (autograd_ctx.py) against
    torch.autograd through the CPU oracle in fp64, same inputs / noise / parameters.  Under contextflow the generalist's
    own parameters are frozen (coupling.py:36 ...) and must receive no gradient - only CN nets and embedding tables
    train; without contextflow (README.md:56) every parameter that takes part trains."""
    import contextflow_amd as cfa
    from tests.helpers import load_specialist
    from tests.gpu_util import set_noise
    name, ctx, ops, M, params, inp = load_specialist(fxname)
    B = inp["x"].shape[0]
    g = torch.Generator().manual_seed(33)
    wts = torch.randn(B, M, generator=g)
    p64 = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in params.items()}
    _, lp = fo.flow_forward(ops, p64, inp["x"].double(), inp["u"].double(), [e.double() for e in inp["eps"]], ctx=ctx,
                            context=inp["context"], cnoise=[c.double() for c in inp["cnoise"]])
    (lp * wts.double()).sum().backward()
    cfg, ds, MM = cfa.preset_config(name)
    cfg.update(generalist=False, enc_emb=ctx["enc_emb"], enc_type=ctx.get("enc_type", "uniform"), contextflow=ctx["contextflow"])
    model = cfa.create_model(cfg, ds, MM, contexts=ctx["contexts"])
    model.load_state_dict(params, strict=True)
    model = model.to(DEV).train()
    set_noise(model, inp["u"], inp["eps"])
    noisy = cfa.layers.UniformCatDequantization if ctx.get("enc_type", "uniform") == "uniform" else cfa.layers.ConditionalGaussianDistribution
    encs = [m for m in model.modules() if isinstance(m, noisy)]
    assert len(encs) == len(inp["cnoise"])
    for e, c in zip(encs, inp["cnoise"]):
        e.fixed_noise = c.to(DEV)
    z, logp = model(inp["x"].to(DEV), inp["context"].to(DEV))
    assert logp.requires_grad
    tol = max(BPD_TOL, 1e-5 * bpd(lp.detach().float(), name).abs().max().item())      # un-normalised without contextflow
    assert (bpd(logp.detach().cpu(), name) - bpd(lp.detach().float(), name)).abs().max() < tol
    (logp * wts.to(DEV)).sum().backward()
    checked = 0
    for k, p in model.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, k
            continue
        if ctx["contextflow"]:
            assert ".CN." in k or "_embeddings" in k or ".context_net." in k, k     # only context parameters train
        ref = p64[k].grad
        if ref is None or float(ref.abs().max()) == 0.0:           # takes no part in this configuration (e.g. Conv1x1.NN)
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, k
        got = p.grad.detach().cpu().double()
        scale = max(ref.abs().max().item(), 1e-3)
        err = (got - ref).abs().max().item() / scale
        assert err < 2e-4, "%s: relative grad error %.3e (scale %.3e)" % (k, err, scale)
        checked += 1
    assert checked >= 20


def test_encoder_noise_is_taped_per_forward(L):
    """Flow-type context encoders (vardeq): the backward replays the Gaussian draw of ITS OWN forward.  Two forwards
    (different injected noise), then the backward of the FIRST: gradients must equal the oracle's for the first forward -
    a draw kept as module state would have been overwritten by the second call."""
    import contextflow_amd as cfa
    from tests.helpers import load_specialist
    from tests.gpu_util import set_noise
    name, ctx, ops, M, params, inp = load_specialist("cifar10_eye_vardeq_cf")
    B = inp["x"].shape[0]
    g = torch.Generator().manual_seed(5)
    wts = torch.randn(B, M, generator=g)
    p64 = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in params.items()}
    _, lp = fo.flow_forward(ops, p64, inp["x"].double(), inp["u"].double(), [e.double() for e in inp["eps"]], ctx=ctx,
                            context=inp["context"], cnoise=[c.double() for c in inp["cnoise"]])
    (lp * wts.double()).sum().backward()
    cfg, ds, MM = cfa.preset_config(name)
    cfg.update(generalist=False, enc_emb=ctx["enc_emb"], enc_type=ctx["enc_type"], contextflow=ctx["contextflow"])
    model = cfa.create_model(cfg, ds, MM, contexts=ctx["contexts"])
    model.load_state_dict(params, strict=True)
    model = model.to(DEV).train()
    set_noise(model, inp["u"], inp["eps"])
    encs = [m for m in model.modules() if isinstance(m, cfa.layers.ConditionalGaussianDistribution)]
    assert len(encs) == len(inp["cnoise"])
    for e, c in zip(encs, inp["cnoise"]):
        e.fixed_noise = c.to(DEV)
    _, logp_a = model(inp["x"].to(DEV), inp["context"].to(DEV))
    for e, c in zip(encs, inp["cnoise"]):                        # second forward: other noise
        e.fixed_noise = (-c.flip(0)).to(DEV)
    _, logp_b = model(inp["x"].to(DEV), inp["context"].to(DEV))
    assert not torch.equal(logp_a, logp_b)
    (logp_a * wts.to(DEV)).sum().backward()                      # backward of the FIRST forward
    checked = 0
    for k, p in model.named_parameters():
        ref = p64[k].grad
        if not p.requires_grad or ref is None or float(ref.abs().max()) == 0.0:
            continue
        scale = max(ref.abs().max().item(), 1e-3)
        err = (p.grad.detach().cpu().double() - ref).abs().max().item() / scale
        assert err < 2e-4, "%s: relative grad error %.3e" % (k, err)
        checked += 1
    assert checked >= 20


@pytest.mark.parametrize("fxname", ["mnist_eye_cf", "mnist_onehot"])
def test_specialist_tape_holds_named_records_and_the_layers_own_cn_path(L, fxname, monkeypatch):
    """The tape a specialist training forward leaves (SpecialistLogProb: first 2 samples of the fixture, injected noise): a flat
    list of layers/_tape.py records, the pre-processing one first, one mixture record per SplitPrior and the final prior's kept
    apart, and the records of the layers the grouped front end served hold the very tensors specialist._front_end returned.
    Then the same step with the front end switched off - every layer forms its own code and CN activations (context.cn_linear /
    cn_chain) - against the same fp64 oracle run, at the tolerances of test_specialist_backward_against_autograd_oracle."""
    import contextflow_amd as cfa
    from contextflow_amd.layers import _tape, autograd_ctx, specialist
    from tests.helpers import load_specialist
    from tests.gpu_util import set_noise
    name, ctx, ops, M, params, inp = load_specialist(fxname)
    B = 2
    x, u, eps, context = inp["x"][:B], inp["u"][:B], [e[:B] for e in inp["eps"]], inp["context"][:B]
    cnoise = [c[:B] for c in inp["cnoise"]]
    wts = torch.randn(B, M, generator=torch.Generator().manual_seed(33))
    p64 = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in params.items()}
    _, lp = fo.flow_forward(ops, p64, x.double(), u.double(), [e.double() for e in eps], ctx=ctx, context=context,
                            cnoise=[c.double() for c in cnoise])
    (lp * wts.double()).sum().backward()
    cfg, ds, MM = cfa.preset_config(name)
    cfg.update(generalist=False, enc_emb=ctx["enc_emb"], enc_type="uniform", contextflow=ctx["contextflow"])
    model = cfa.create_model(cfg, ds, MM, contexts=ctx["contexts"])
    model.load_state_dict(params, strict=True)
    model = model.to(DEV).train()
    set_noise(model, u, eps)
    encs = [m for m in model.modules() if isinstance(m, cfa.layers.UniformCatDequantization)]
    assert len(encs) == len(cnoise)
    for e, c in zip(encs, cnoise):
        e.fixed_noise = c.to(DEV)
    served, real = [], specialist._front_end
    monkeypatch.setattr(specialist, "_front_end", lambda *a, **k: served.append(real(*a, **k)) or served[-1])
    ctx_layers = [m for m in model.sequence_modules if getattr(m, "context_net", None)]
    nsplit = sum(isinstance(m, cfa.layers.SplitPrior) for m in model.sequence_modules)

    def step():
        """one training step: the tape of its forward, after logp and every gradient passed the oracle's check"""
        model.zero_grad(set_to_none=True)
        _, logp = model(x.to(DEV), context.to(DEV))
        fn = logp.grad_fn
        tape, prior = list(fn.tape), fn.prior
        assert all(type(r) in autograd_ctx.RECORDS for r in tape + [prior]), [type(r) for r in tape]
        assert [type(r) is _tape.Pre for r in tape] == [True] + [False] * (len(tape) - 1)
        assert sum(type(r) is _tape.CtxMixture for r in tape) == nsplit
        assert type(prior) is _tape.CtxMixture and prior.dist is model.dist
        assert [r.module for r in tape if hasattr(r, "module")] == ctx_layers
        tol = max(BPD_TOL, 1e-5 * bpd(lp.detach().float(), name).abs().max().item())
        assert (bpd(logp.detach().cpu(), name) - bpd(lp.detach().float(), name)).abs().max() < tol
        (logp * wts.to(DEV)).sum().backward()
        checked = 0
        for k, p in model.named_parameters():
            if not p.requires_grad:
                assert p.grad is None, k
                continue
            ref = p64[k].grad
            if ref is None or float(ref.abs().max()) == 0.0:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
                continue
            assert p.grad is not None, k
            scale = max(ref.abs().max().item(), 1e-3)
            err = (p.grad.detach().cpu().double() - ref).abs().max().item() / scale
            assert err < 2e-4, "%s: relative grad error %.3e (scale %.3e)" % (k, err, scale)
            checked += 1
        assert checked >= 20
        return tape

    tape = step()
    pre = served[-1]
    hit = 0
    for r in tape:
        e = pre.get(id(getattr(r, "module", None)))
        if e is None:
            continue
        hit += 1
        assert r.c is e.c and e.c is not None and e.logp is not None
        if type(r) is _tape.CtxAffine:
            assert r.m is e.m
        else:
            assert r.a1 is e.a1 and r.a2 is e.a2 and r.cn is e.cn
    assert hit == len(pre) == len(ctx_layers)             # uniform encoders, conv couplings: the front end serves every layer
    monkeypatch.setattr(specialist, "FRONT_END", False)
    tape = step()
    assert served[-1] == {} and all(r.c is not None for r in tape if hasattr(r, "module"))


@pytest.mark.parametrize("name,contexts,emb,typ,cflow", [
    ("mnist", [64], "eye", "uniform", False),            # README.md:56
    ("cifar10", [15, 5], "onehot", "vardeq", False),     # README.md:61
    ("atm", [68], "onehot", "vardeq", True),             # README.md:66
    ("atm", [68], "eye", "argmax", True),                # README.md:67
    ("atm", [68], "embed", "probsample", True),          # README.md:69
])
def test_specialist_training_modes_of_the_readme(L, name, contexts, emb, typ, cflow):
    """A few AdamW steps of the specialist training modes the reference's README lists that have no gradient fixture of their
    own (the per-layer backward pieces are pinned by test_specialist_backward_against_autograd_oracle): the loss stays
    finite and improves, every trainable tensor that takes part receives a finite gradient."""
    import contextflow_amd as cfa
    torch.manual_seed(0)
    cfg, ds, M = cfa.preset_config(name)
    cfg.update(generalist=False, enc_emb=emb, enc_type=typ, contextflow=cflow)
    model = cfa.create_model(cfg, ds, M, contexts=contexts).to(DEV)
    g = torch.Generator().manual_seed(11)
    B = 24
    x = torch.rand(B, *ds, generator=g) if name == "atm" else torch.randint(0, 256, (B, *ds), generator=g).float()
    ctx = torch.stack([torch.randint(0, k, (B,), generator=g) for k in contexts], 1)
    gt = torch.randint(0, M, (B,), generator=g)
    x, ctx, gt = x.to(DEV), ctx.to(DEV), gt.to(DEV)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=5e-4)
    dim_inv = 1.0 / (ds[0] * ds[1] * ds[2])
    losses = []
    for it in range(8):
        opt.zero_grad(set_to_none=True)
        logp = dim_inv * model.log_prob(x, ctx)
        assert logp.requires_grad
        loss = torch.nn.functional.cross_entropy(logp, gt)
        loss.backward()
        if it == 0:
            got = [p for p in params if p.grad is not None]
            assert len(got) >= 20 and all(torch.isfinite(p.grad).all() for p in got)
        opt.step()
        losses.append(float(loss.detach()))
    assert all(math.isfinite(v) for v in losses), losses
    assert min(losses[1:]) < losses[0], losses            # the encoders draw fresh noise every step: the loss is stochastic


@pytest.mark.parametrize("name,channels", [("msl", 55), ("smd", 38)])
def test_other_timeseries_presets_match_oracle(L, name, channels):
    """MSL / SMD (model.py:211-216): the SMAP topology with 55 / 38 sensor channels - transformer width 112 / 80 is
    beyond the fused ViT kernel (dim <= 64), so the layer-by-layer ViT kernels run; checked against the oracle (which the
    reference fixtures pin on the same code path for SMAP)."""
    import contextflow_amd as cfa
    from oracle import params as op
    ds = (channels, 8, 1)
    ops, prior_size, M = fo.program("smap", data_size=ds)
    spec = op.param_spec(ops, prior_size, M)
    params = op.gen_params(spec, 3)
    g = torch.Generator().manual_seed(8)
    B = 5
    x = torch.rand(B, *ds, generator=g)
    eps = [torch.randn(B, 1, 8, 1, generator=g)] if channels % 2 else []
    p_or = {k: v.clone() for k, v in params.items()}
    _, lp_ref = fo.flow_forward(ops, p_or, x, None, eps, init_actnorm=True)
    cfg, ds2, MM = cfa.preset_config(name)
    assert tuple(ds2) == ds and MM == M
    model = cfa.create_model(cfg, ds2, MM)
    assert list(model.state_dict().keys()) == list(spec.keys())
    model.load_state_dict(params, strict=True)
    model = model.to(DEV).eval()
    from tests.gpu_util import set_noise
    set_noise(model, None, eps)
    with torch.no_grad():
        _, lp1 = model(x.to(DEV))                   # first call: ActNorm init, layer by layer
        set_noise(model, None, eps)
        _, lp2 = model(x.to(DEV))                   # fused plan
    D = channels * 8
    for lp in (lp1, lp2):
        assert (fo.bits_per_dim(lp.cpu(), D) - fo.bits_per_dim(lp_ref, D)).abs().max().item() < 2e-5


@pytest.mark.parametrize("tag,D,krn,pad", [("maf_3x3", 6, (3, 3), (1, 1)), ("maf_3x1", 8, (3, 1), (1, 0))])
def test_masked_coupling_matches_reference(L, tag, D, krn, pad):
    """MaskedCoupling (--coupling maf, ar.py:15-57) through the generic reflect-padded conv kernels against the
    reference layer's outputs; the masks multiply the weights in place, as upstream."""
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "unit_maf.npz"))
    m = L.MaskedCoupling(D, kernel_size=krn, padding=pad)
    m.load_state_dict({k[len(tag) + 4:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith(tag + "/sd:")}, strict=True)
    m = m.to(DEV)
    z, ldj = m(torch.from_numpy(fx[tag + "/x"]).to(DEV))
    assert (z.cpu() - torch.from_numpy(fx[tag + "/z"])).abs().max() < 2e-5
    assert (ldj.cpu() - torch.from_numpy(fx[tag + "/ldj"])).abs().max() < 2e-4
    with pytest.raises(NotImplementedError):
        m.reverse(z)


@pytest.mark.parametrize("B,Cin,Cout,H,W,krn", [(3, 5, 70, 7, 5, (3, 3)), (4, 13, 52, 8, 1, (3, 1)), (2, 32, 32, 16, 16, (3, 3)),
                                                 (5, 8, 24, 6, 9, (1, 1)), (2, 128, 128, 4, 4, (3, 3)), (1, 3, 40, 2, 2, (3, 3))])
def test_generic_conv_and_its_backward(L, B, Cin, Cout, H, W, krn):
    """The shape-agnostic convolution (implicit GEMM on the fp32 matrix cores, reflect padding) against torch in fp64, and
    its backward - zero-padded transposed convolution + adjoint of the reflect padding for the data, split-K GEMM over
    the unfolded rows for the weights - against fp64 autograd."""
    from contextflow_amd.layers.autograd_layers import conv_backward
    from contextflow_amd.layers.coupling import conv2d_reflect
    pad = (krn[0] // 2, krn[1] // 2)
    g = torch.Generator().manual_seed(B * 100 + Cin)
    conv = torch.nn.Conv2d(Cin, Cout, krn, padding=pad, padding_mode="reflect")
    x = torch.randn(B, Cin, H, W, generator=g)
    gy = torch.randn(B, Cout, H, W, generator=g)
    c64 = torch.nn.Conv2d(Cin, Cout, krn, padding=pad, padding_mode="reflect").double()
    c64.load_state_dict({k: v.double() for k, v in conv.state_dict().items()})
    x64 = x.double().requires_grad_(True)
    y64 = c64(x64)
    y64.backward(gy.double())
    conv = conv.to(DEV)
    for relu in (False, True):
        y = conv2d_reflect(x.to(DEV), conv, relu)
        ref = torch.relu(y64) if relu else y64
        close(y, ref.detach(), tol=2e-5)
    grads = {}
    gx = conv_backward(x.to(DEV), conv, gy.to(DEV), grads)
    close(gx, x64.grad, tol=2e-5)
    close(grads[conv.weight], c64.weight.grad, tol=2e-5)
    close(grads[conv.bias], c64.bias.grad, tol=2e-5)


@pytest.mark.parametrize("kind", ["maf_3x3", "maf_3x1", "coupling_3x1", "coupling_3x3"])
def test_conv_coupling_backward_against_autograd_oracle(L, kind):
    """Backward of the layers whose conditioner runs on the generic conv kernels - MaskedCoupling (--coupling maf, ar.py:15-57)
    and Coupling with kernels / shapes outside the fused step kernels (--coupling conv on time series, model.py:114) -
    against torch.autograd through the fp64 oracle.  MaskedCoupling: the weights are masked in place (masked_conv_2d.py:22),
    so the reference's autograd returns the plain convolution gradient: the oracle runs on the pre-masked weights with the
    masks set to one."""
    from contextflow_amd.layers.autograd_layers import layer_backward
    g = torch.Generator().manual_seed(11)
    if kind.startswith("maf"):
        D, krn, pad = (6, (3, 3), (1, 1)) if kind == "maf_3x3" else (8, (3, 1), (1, 0))
        fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "unit_maf.npz"))
        sd = {k[len(kind) + 4:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith(kind + "/sd:")}
        m = L.MaskedCoupling(D, kernel_size=krn, padding=pad)
        m.load_state_dict(sd, strict=True)
        x = torch.from_numpy(fx[kind + "/x"])
        p = {}
        for k, v in sd.items():
            p["0." + k] = v.double()
        for c in ("conv1", "conv2", "conv3"):                       # pre-masked weights, masks of ones
            p["0.NN.%s.weight" % c] = (sd["NN.%s.weight" % c] * sd["NN.%s.mask" % c]).double().requires_grad_(True)
            p["0.NN.%s.bias" % c] = sd["NN.%s.bias" % c].double().requires_grad_(True)
            p["0.NN.%s.mask" % c] = torch.ones_like(sd["NN.%s.mask" % c]).double()
        x64 = x.double().requires_grad_(True)
        z64, l64 = fo.masked_coupling_fwd(x64, p, "0.", pad)
    else:
        t, sd = unit(kind)
        C = t["x"].shape[1]
        krn, pad = tuple(int(v) for v in t["krn"]), tuple(int(v) for v in t["pad"])
        m = L.Coupling(C, kernel_size=krn, padding=pad)
        m.load_state_dict(sd)
        x = t["x"]
        p = {"0." + k: v.double().requires_grad_(True) for k, v in sd.items()}
        x64 = x.double().requires_grad_(True)
        z64, l64 = fo.coupling_fwd(x64, p, "0.", pad)
    gz = torch.randn(z64.shape, generator=g)
    gld = torch.randn(x.shape[0], generator=g)
    ((z64 * gz.double()).sum() + (l64 * gld.double()).sum()).backward()
    m = m.to(DEV)
    gx, grads = layer_backward(m, x.to(DEV), gz.to(DEV), gld.to(DEV))
    close(gx, x64.grad, tol=5e-5)
    checked = 0
    for name, prm in m.named_parameters():
        ref = p["0." + name].grad
        assert prm in grads, name
        scale = max(ref.abs().max().item(), 1e-3)
        err = (grads[prm].detach().cpu().double() - ref).abs().max().item() / scale
        assert err < 1e-4, (name, err)
        checked += 1
    assert checked == 6


def test_in_kernel_noise_follows_torch_seed(L):
    """The position of the in-kernel Philox stream is drawn from torch's CUDA generator once per forward: re-seeding
    reproduces the noise (as `torch.manual_seed` does for the reference's torch.rand / randn draws), another seed gives
    other noise - eagerly and through the auto-captured graph (torch registers the generator with the graph)."""
    from tests.gpu_util import build_model
    ops, _, M, params, fx = load_e2e("mnist")
    model = build_model("mnist", params)
    x = torch.randint(0, 256, (32, 1, 32, 32), generator=torch.Generator().manual_seed(1)).float().to(DEV)

    def run(seed, n, user_draws=0):
        torch.manual_seed(seed)
        for _ in range(user_draws):                                  # the user's own use of the CUDA generator between the
            torch.randn(17, device=DEV)                              # re-seed and the forward must not hide the re-seed
        with torch.no_grad():
            return [model.log_prob(x).clone() for _ in range(n)]
    a = run(7, 5)            # calls 3.. replay a captured graph
    b = run(7, 5)
    c = run(8, 2)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert not torch.equal(a[0], a[1])                               # successive calls draw fresh noise
    assert not torch.equal(a[0], c[0])
    d, e = run(7, 3, user_draws=2), run(7, 3, user_draws=2)
    for u, v in zip(d, e):
        assert torch.equal(u, v)
    assert not torch.equal(d[0], a[0])                               # the stream position follows torch's generator


def test_in_kernel_noise_statistics(L):
    """cf_preprocess_rng_fwd (Philox inside the kernel): the implied dequantisation noise is U[0,1), the Augment channel
    N(0,1), the log-det equals the one the explicit-noise kernel gives for that very noise, and consecutive calls (and
    therefore graph replays) draw fresh noise."""
    from contextflow_amd.layers import _hip
    B, C, H, W = 64, 3, 32, 32
    N, A = C * H * W, H * W
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (B, C, H, W), generator=g).float().to(DEV)
    t1, s1, t2, s2 = 0.0, 256.0, 1e-4, 1.0 / (1.0 - 2e-4)
    cst = -N * math.log(s1) - N * math.log(s2)
    state = torch.zeros(1, device=DEV, dtype=torch.int64)
    outs = []
    for _ in range(2):
        y = torch.empty(B, C + 1, H, W, device=DEV)
        ldj = torch.empty(B, device=DEV)
        _hip.call("cf_preprocess_rng_fwd", _hip.p(x), _hip.p(y), _hip.p(ldj), _hip.p(state), 1234, B, N, A, (C + 1) * H * W,
                  t1, s1, t2, s2, cst, 1, _hip.stream())
        outs.append((y, ldj))
    assert int(state.item()) == 2
    y, ldj = outs[0]
    v = torch.sigmoid(y[:, :C].double())                          # v = ((x+u)/256)(1-2a) + a
    u = ((v - t2) * s2 - t1) * s1 - x.double()
    assert u.min() > -1e-3 and u.max() < 1 + 1e-3
    assert abs(u.mean().item() - 0.5) < 5e-3 and abs(u.var().item() - 1 / 12) < 2e-3
    eps = y[:, C:].double()
    assert abs(eps.mean().item()) < 2e-2 and abs(eps.var().item() - 1.0) < 3e-2
    assert abs((eps ** 3).mean().item()) < 5e-2 and abs((eps ** 4).mean().item() - 3.0) < 0.15
    ref = cst + (-torch.log(v) - torch.log1p(-v)).flatten(1).sum(-1) + (0.5 * eps ** 2 + 0.5 * math.log(2 * math.pi)).flatten(1).sum(-1)
    assert (ldj.double().cpu() - ref.cpu()).abs().max() < 2e-2
    assert (outs[1][0] - y).abs().max() > 0.1                     # second call: different noise
    # correlation between neighbouring pixels / samples of the uniforms is absent
    uu = u.flatten(1)
    c1 = torch.corrcoef(torch.stack([uu[:, :-1].flatten(), uu[:, 1:].flatten()]))[0, 1].abs().item()
    c2 = torch.corrcoef(torch.stack([uu[:-1].flatten(), uu[1:].flatten()]))[0, 1].abs().item()
    assert c1 < 1e-2 and c2 < 1e-2


def test_large_launch_equals_chunked(L):
    """One 262 144-sample call (4.3e9 activation elements per tensor: beyond 32-bit element indices) gives exactly the
    rows that four 65 536-sample calls give on the same inputs and noise - the bench's default chunk size is safe."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e("cifar10")
    model = build_model("cifar10", params).eval()
    B, step = 262144, 65536
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randint(0, 256, (B, 3, 32, 32), device=DEV, generator=g, dtype=torch.int32).float()
    u = torch.rand(B, 3, 32, 32, device=DEV, generator=g)
    eps = torch.randn(B, 1, 32, 32, device=DEV, generator=g)
    with torch.no_grad():
        set_noise(model, u, [eps])
        _, big = model(x)
        big = big.clone()
        for c0 in range(0, B, step):
            set_noise(model, u[c0:c0 + step], [eps[c0:c0 + step]])
            _, part = model(x[c0:c0 + step])
            assert torch.equal(part, big[c0:c0 + step]), c0
    assert torch.isfinite(big).all()


# ------------------------------------------------------------------------------------------ RCCL (one rank)
_RCCL_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["CF_ROOT"])
import torch, torch.distributed as dist
import contextflow_amd as cfa
from contextflow_amd import dist as cdist
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1)          # backend "nccl" is RCCL on ROCm
assert dist.get_backend() == "nccl"
dev = torch.device("cuda", 0)

def build():
    torch.manual_seed(0)                                         # also restarts the in-kernel noise stream: both runs draw the same noise
    cfg, ds, M = cfa.preset_config("mnist")
    return cfa.create_model(cfg, ds, M).to(dev), ds, M

x = torch.randint(0, 256, (64, 1, 32, 32), generator=torch.Generator().manual_seed(1)).float().to(dev)
gt = torch.randint(0, 10, (64,), generator=torch.Generator().manual_seed(2)).to(dev)

def run(collectives):
    os.environ["CF_DIST_SINGLE_RANK"] = "1" if collectives else "0"
    model, ds, M = build()
    with torch.no_grad():
        if collectives:
            with cdist.sharded_actnorm_init():                  # all-reduce of fp64 [sum x | sum x^2 | n] per ActNorm
                model(x)
        else:
            model(x)
    cdist.broadcast_parameters(model, src=0)                    # one flat broadcast per dtype (fp32, int64)
    _, logp = model(x)
    loss = torch.nn.functional.cross_entropy(logp / 1024.0, gt)
    loss.backward()
    cdist.allreduce_gradients(model)                            # bucketed fp32 all-reduce
    red = cdist.allreduce_nll(torch.logsumexp(logp.detach(), -1).sum().double(), 64)     # fp64 [sum log p, count]
    return red.cpu(), {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}, \
        {k: v.detach().cpu() for k, v in model.state_dict().items()}

r1, g1, s1 = run(True)
r0, g0, s0 = run(False)
assert torch.equal(r1, r0), (r1, r0)
assert g1.keys() == g0.keys() and len(g1) > 20
for k in s0:
    assert torch.allclose(s1[k].double(), s0[k].double(), rtol=1e-6, atol=1e-7), k     # sums path vs two-pass init
for k in g0:
    assert torch.allclose(g1[k], g0[k], rtol=2e-4, atol=1e-7), k
torch.cuda.synchronize()
dist.destroy_process_group()
print("RCCL_OK", ".".join(str(v) for v in torch.cuda.nccl.version()))
'''


@pytest.mark.gpu
def test_rccl_communicator_runs_every_collective_of_the_data_parallel_path(tmp_path):
    """No multi-GPU node is available to the build, so the RCCL calls of contextflow_amd.dist run here through a real
    communicator of ONE rank on the one GPU (CF_DIST_SINGLE_RANK=1): the sharded ActNorm init (fp64 all-reduce), the flat
    fp32 / int64 parameter broadcast, the bucketed gradient all-reduce and the fp64 NLL all-reduce - dtypes, reduce ops and
    CUDA-tensor plumbing as in an N-rank job - and must leave the numbers of a run without collectives unchanged."""
    import subprocess
    import sys
    script = tmp_path / "rccl_worker.py"
    script.write_text(_RCCL_WORKER)
    env = dict(os.environ, CF_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", RANK="0", WORLD_SIZE="1",
               LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RCCL_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


_DP_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["CF_ROOT"])
import torch, torch.distributed as dist
import contextflow_amd as cfa
from contextflow_amd import dist as cdist
torch.cuda.set_device(0)
rank, world, backend = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), os.environ["DP_BACKEND"]
dist.init_process_group(backend, rank=rank, world_size=world)
dev = torch.device("cuda", 0)
name = os.environ.get("DP_FLOW", "cifar10")
cfg, ds, M = cfa.preset_config(name)
B = int(os.environ.get("DP_BATCH", "64")) * world                # global batch; every rank owns a contiguous share
g = torch.Generator().manual_seed(1)
xg = (torch.rand(B, *ds, generator=g) if name == "smap" else torch.randint(0, 256, (B, *ds), generator=g).float()).to(dev)
ug = torch.rand(B, *ds, generator=g).to(dev)
eg = torch.randn(B, 1, ds[1], ds[2], generator=g).to(dev)
yg = torch.randint(0, M, (B,), generator=g).to(dev)
inv = 1.0 / xg[0].numel()
loss_fn = lambda lp, y: torch.nn.functional.cross_entropy(lp * inv, y) if M > 1 else -(lp * inv).mean()

def set_noise(m, lo, hi):                                        # the same noise on every path: rows lo..hi of the global draw
    for q in m.sequence_modules:
        if isinstance(q, cfa.layers.Dequantization):
            q.dist.fixed_noise = ug[lo:hi]
        if isinstance(q, cfa.layers.Augment):
            q.distribution.fixed_noise = eg[lo:hi]

def build(lo, hi):
    torch.manual_seed(0)
    m = cfa.create_model(cfg, ds, M).to(dev)
    set_noise(m, 0, B)
    with torch.no_grad():
        m(xg)                                                    # ActNorm init on the GLOBAL batch, identical on every rank
    set_noise(m, lo, hi)
    return m.train()

lo, hi = cdist.shard_bounds(B, rank, world)
mode = os.environ["DP_MODE"]
if mode == "two_rank_eager":
    # every rank: one eager data-parallel step on ITS shard; gradients = the one-process gradients on the whole batch
    os.environ["CF_DIST_SINGLE_RANK"] = "0"
    dp = build(lo, hi)
    dp.data_parallel = True
    loss = loss_fn(dp.log_prob(xg[lo:hi]), yg[lo:hi])
    loss.backward()
    bucket = dp._grad_bucket
    assert bucket is not None and len(bucket.segments) >= 2
    for p in dp.parameters():
        assert p.grad is not None and p.grad.data_ptr() == bucket.view(p).data_ptr()      # views of the flat bucket, no copies
    ref = build(0, B)                                            # one process, concatenated batch, no collectives
    loss_fn(ref.log_prob(xg), yg).backward()
    worst = 0.0
    for (k, a), (_, b) in zip(dp.named_parameters(), ref.named_parameters()):
        d = (a.grad - b.grad).abs().max().item() / max(b.grad.abs().max().item(), 1e-30)
        worst = max(worst, d)
        assert d < 2e-6, (k, d)
    print("rank %d: worst relative gradient difference %.2e over %d tensors, %d messages of %s bytes"
          % (rank, worst, len(list(dp.parameters())), len(bucket.segments), bucket.message_bytes()))
else:
    # one rank, RCCL: the captured data-parallel step (collectives inside the graph) against the eager loop without collectives
    assert backend == "nccl" and world == 1
    os.environ["CF_DIST_SINGLE_RANK"] = "0"
    eager = build(0, B)
    opt_e = torch.optim.AdamW(eager.parameters(), lr=1e-3, fused=True, capturable=True)
    losses_e = []
    for _ in range(4):
        opt_e.zero_grad(set_to_none=True)
        l = loss_fn(eager.log_prob(xg), yg)
        l.backward()
        opt_e.step()
        losses_e.append(float(l.detach()))
    os.environ["CF_DIST_SINGLE_RANK"] = "1"                     # a one-rank RCCL communicator carries the collectives
    cap = build(0, B)
    opt_c = torch.optim.AdamW(cap.parameters(), lr=1e-3, fused=True, capturable=True)
    step = cap.capture_train_step(xg, loss_fn, opt_c)            # data_parallel defaults to "a communicator is active"
    assert cap.data_parallel
    losses_c = [float(step(xg, yg).detach()) for _ in range(4)]
    for p in cap.parameters():
        assert p.grad.data_ptr() == cap._grad_bucket.view(p).data_ptr()
    for a, b in zip(losses_e, losses_c):
        assert abs(a - b) < 2e-6 * max(1.0, abs(a)), (losses_e, losses_c)
    for (k, a), (_, b) in zip(eager.named_parameters(), cap.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), k           # same kernels, same order: the bucket only changes where gradients live
    print("captured data-parallel step == eager loop, losses", losses_c)
torch.cuda.synchronize()
dist.barrier()
dist.destroy_process_group()
print("DP_OK")
'''


def _run_dp_workers(tmp_path, world, backend, mode, flow, port, batch=64):
    import subprocess
    import sys
    script = tmp_path / "dp_worker.py"
    script.write_text(_DP_WORKER)
    env = dict(os.environ, CF_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0", DP_BACKEND=backend, DP_MODE=mode, DP_FLOW=flow, DP_BATCH=str(batch))
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK="0"), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 and "DP_OK" in o for p, o in zip(procs, outs)), "\n".join(o[-3000:] for o in outs)
    print(outs[0][-600:])


@pytest.mark.gpu
@pytest.mark.parametrize("flow", ["cifar10", "smap"])
def test_data_parallel_step_of_two_ranks_equals_one_process_on_the_whole_batch(tmp_path, flow):
    """SURVEY.md 8(f)1 "+ gradient all-reduce" (experiment_cl.py:130-136 on N ranks): two processes (both on device 0, gloo
    transport - a one-GPU box), each with its contiguous half of a batch of 128, run ONE eager data-parallel step
    (FlowSequential.data_parallel: gradients written into the flat bucket, all-reduced segment by segment during the
    backward, averaged); every gradient tensor equals the one a single process computes on the whole batch to 2e-6 of its
    largest entry (two split-K halves averaged against one sum: rounding only)."""
    _run_dp_workers(tmp_path, 2, "gloo", "two_rank_eager", flow, 29551 if flow == "cifar10" else 29553)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [64, 1100])
def test_captured_data_parallel_step_through_rccl_equals_the_eager_loop(tmp_path, batch):
    """The data-parallel training step as ONE HIP graph with its collectives captured inside, through a real RCCL
    communicator (of one rank: a one-GPU box): four updates give bit for bit the parameters of the eager loop without any
    collective, and p.grad are views of the flat bucket (no concatenation, no copy back).  64 samples: the weight gradients and
    the collectives are issued on the flow's side stream (autograd.WGRAD_SIDE_MAX_BATCH); 1100: on the main stream."""
    _run_dp_workers(tmp_path, 1, "nccl", "one_rank_captured", "cifar10", 29555 + (batch > 64), batch)


# ------------------------------------------------------------------------------------------ Winograd form of the 3x3
@pytest.mark.parametrize("tag", [None, "stress", "extreme"])
@pytest.mark.parametrize("name", ["mnist", "cifar10"])
def test_e2e_at_saturating_batch_runs_the_winograd_kernels(L, name, tag):
    """At the batch sizes the benchmark runs (>= 4096 samples per call) every resolution level takes the Winograd
    F(2x2,3x3) form of the coupling net's 3x3 (cf_step_common.h: winograd_phase2; small batches take the direct form at
    8x8 / 4x4).  The fixture's samples and captured noise, repeated to 4096 rows, must reproduce the reference's
    per-sample log-densities within the same bits/dim bar as the small-batch test, in every parameter regime."""
    from tests.gpu_util import build_model, set_noise
    ops, _, M, params, fx = load_e2e(name, tag)
    x, u, eps = e2e_inputs(name, fx)
    rep = 4096 // x.shape[0]
    tol = stress_tolerance(fx, tag) if tag else BPD_TOL
    model = build_model(name, params)
    set_noise(model, u.repeat(rep, 1, 1, 1), [e.repeat(rep, *([1] * (e.dim() - 1))) for e in eps])
    z, logp = model(x.repeat(rep, 1, 1, 1).to(DEV))
    ref = torch.from_numpy(fx["logp"]).repeat(rep, 1)
    d32 = (bpd(logp.cpu(), name) - bpd(ref, name)).abs().max().item()
    print("%s %s B=%d: |d bits/dim| vs reference fp32 %.2e (bar %.1e)" % (name, tag, x.shape[0] * rep, d32, tol))
    assert d32 < tol
    if "logp_f64" in fx:
        ref64 = torch.from_numpy(fx["logp_f64"]).repeat(rep, 1)
        assert (bpd(logp.cpu(), name) - bpd(ref64, name)).abs().max().item() < tol
    zr = torch.from_numpy(fx["z"]).repeat(rep, 1, 1, 1)
    assert (z.cpu() - zr).abs().max().item() <= 2e-4 * max(1.0, zr.abs().max().item())


@pytest.mark.parametrize("tag", [None, "stress", "extreme", "wide"])
def test_e2e_at_saturating_batch_runs_the_wave_kernel(L, tag):
    """The SMAP counterpart of the test above.  Batches above TransCoupling.STEP_RS_MAX_BATCH take the wave form of the
    one-kernel transformer step (cf_vit_step_fwd: 8 samples per wave, everything in registers) - the kernel behind the SMAP
    benchmark line - while every fixture-sized batch takes the row-split form.  The fixtures' rows and captured noise are
    tiled past that threshold (the last workgroup partially filled) and every row must reproduce the reference's
    per-sample log-density within the bars of the small-batch tests; "wide" = 512 distinct samples
    (tests/golden/e2e_smap_wide.npz), where the reference's own fp32 answer is up to 6.9e-6 bits/dim from its fp64 run."""
    from tests.gpu_util import build_model, set_noise
    from contextflow_amd.layers.coupling import TransCoupling
    ops, _, M, params, fx = load_e2e("smap", None if tag == "wide" else tag)
    if tag == "wide":
        fx = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "e2e_smap_wide.npz")))
    x, u, eps = e2e_inputs("smap", fx)
    n0 = x.shape[0]
    rep = 8192 // n0 + 1
    B = n0 * rep - 3                                           # ragged: the last wave / workgroup is partially filled
    tol = stress_tolerance(fx, tag) if tag in ("stress", "extreme") else BPD_TOL
    model = build_model("smap", params)
    assert B > TransCoupling.STEP_RS_MAX_BATCH
    assert all(m.step_variant(B) == "wave" for m in model.sequence_modules if isinstance(m, TransCoupling))
    set_noise(model, None, [e.repeat(rep, 1, 1, 1)[:B] for e in eps])
    with torch.no_grad():
        z, logp = model(x.repeat(rep, 1, 1, 1)[:B].to(DEV))
    ref = torch.from_numpy(fx["logp"]).repeat(rep, 1)[:B]
    ref64 = torch.from_numpy(fx["logp_f64"]).repeat(rep, 1)[:B]
    e32 = (bpd(logp.cpu(), "smap") - bpd(ref, "smap")).abs()
    e64 = (bpd(logp.cpu(), "smap") - bpd(ref64, "smap")).abs()
    print("smap %s B=%d wave form: |d bits/dim| vs reference fp32 max %.2e rms %.2e, vs its fp64 run max %.2e rms %.2e (bar %.1e; "
          "reference fp32 vs fp64 %.2e)" % (tag, B, e32.max(), e32.pow(2).mean().sqrt(), e64.max(), e64.pow(2).mean().sqrt(), tol,
                                            (bpd(ref, "smap") - bpd(ref64, "smap")).abs().max()))
    assert e32.max().item() < tol and e64.max().item() < tol
    # every copy of a fixture row gives the same bits: the result does not depend on the position in the batch
    lp = logp.cpu()
    assert (lp[n0:2 * n0] - lp[:n0]).abs().max() == 0 and (lp[B - n0:] - lp[(B - n0) % n0:][:n0]).abs().max() == 0
    if "z" in fx:
        zr = torch.from_numpy(fx["z"]).repeat(rep, 1, 1, 1)[:B]
        assert (z.cpu() - zr).abs().max().item() <= 2e-4 * max(1.0, zr.abs().max().item())


@pytest.mark.parametrize("squeeze", [False, True])
@pytest.mark.parametrize("C,H", [(8, 16), (16, 16), (32, 8), (64, 4)])
def test_winograd_step_kernel_against_the_oracle(L, C, H, squeeze):
    """One fused step through the production entry point at a batch that selects the Winograd kernels (4100 samples: the
    last workgroup is partially filled), against the oracle of the same step and against the direct-form kernel: z to
    1e-5 of its scale, the log-det to 1e-5 relative - the bars of test_fused_step_phases."""
    from tests.gpu_util import fused_step_debug
    B, W = 4100, H
    torch.manual_seed(C * 1000 + 7)
    conv, act, cpl = L.Conv1x1((C, H, W)), L.ActNorm((C, H, W)), L.Coupling(C, kernel_size=(3, 3), padding=(1, 1))
    with torch.no_grad():
        conv.NN.add_(0.1 * torch.randn(C, C))
        act.NN_t.copy_(0.3 * torch.randn(C)); act.NN_logs.copy_(0.2 * torch.randn(C)); act.initialized.fill_(1)
    act._init_done = True
    x = torch.randn(B, C, H, W)
    p = {"0." + k: v.detach().double() for k, v in cpl.state_dict().items()}
    y, l0 = fo.conv1x1_fwd(x.double(), conv.NN.detach().double())
    y, l1 = fo.actnorm_fwd(y, act.NN_t.detach().double(), act.NN_logs.detach().double())
    zref, l2 = fo.coupling_fwd(y, p, "0.", (1, 1))
    for m in (conv, act, cpl):
        m.to(DEV)
    xin = fo.squeeze_inv(x, (2, 2)) if squeeze else x
    z, ldj, d = fused_step_debug(xin.to(DEV).contiguous(), conv, act, cpl, squeeze=squeeze)
    scale = max(1.0, zref.abs().max().item())
    for got in (d["z_prod"], z):                          # Winograd form (production at this batch), direct form (dump kernel)
        assert (got.cpu().double() - zref).abs().max().item() <= 1e-5 * scale
    lref = l0 + l1 + l2
    for got in (d["ldj_prod"], ldj):
        assert ((got.cpu().double() - lref).abs() / lref.abs().clamp_min(1.0)).max().item() <= 1e-5


def test_taped_training_step_at_a_large_batch_is_clean(L):
    """Regression (round 2): plane stores through a buffer resource with a scalar offset were followed by a VALU write of
    their data registers; from ~9000 samples per launch a few rows of the gradient planes carried register garbage
    (1e20-1e38) and the 3x3 weight gradients blew up, intermittently.  Six training backward passes at 9216 samples (the
    Winograd form of the taping forward at every level): all gradients finite and EQUAL to those of the form that rebuilds
    the tape at backward time - round 2's recompute rebuilt h2 in the direct form, flipped ReLU masks of units within
    rounding of zero and needed a 1e-2 bar here."""
    import contextflow_amd as cfa
    from contextflow_amd.layers import flowsequential as fs
    B = 9216
    torch.manual_seed(0)
    cfg, ds, M = cfa.preset_config("cifar10")
    model = cfa.create_model(cfg, ds, M).to(DEV)
    x = torch.randint(0, 256, (B, *ds), device=DEV).float()
    gt = torch.randint(0, M, (B,), device=DEV)
    with torch.no_grad():
        model(x[:256])

    def grads(tape):
        prev, fs.TAPE_PLANES = fs.TAPE_PLANES, tape
        try:
            model.zero_grad(set_to_none=True)
            torch.manual_seed(1)
            _, lp = model(x)
            torch.nn.functional.cross_entropy(lp / 3072.0, gt).backward()
            torch.cuda.synchronize()
            return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        finally:
            fs.TAPE_PLANES = prev
    ref = grads(False)
    for _ in range(6):
        g = grads(True)
        for k in ref:
            assert torch.isfinite(g[k]).all(), k
            assert (g[k] - ref[k]).abs().max().item() <= 1e-5 * ref[k].abs().max().item(), k   # measured: bitwise equal


@pytest.mark.parametrize("fxname", ["mnist_eye_cf", "cifar10_onehot_cf", "cifar10_eye"])
def test_specialist_forward_at_saturating_batch_runs_the_winograd_kernels(L, fxname):
    """The specialist step kernels (per-sample bias on the conditioner output / before its first ReLU) take the Winograd
    form of the 3x3 at 8x8 / 4x4 only from 1024 / 2048 samples per call: the fixture's rows, noise and contexts repeated
    to 4096 samples must give the reference's log-densities within the same bar as the small-batch test."""
    import contextflow_amd as cfa
    from tests.helpers import load_specialist
    from tests.gpu_util import set_noise
    name, ctx, ops, M, params, inp = load_specialist(fxname)
    cfg, ds, MM = cfa.preset_config(name)
    enc_type = ctx.get("enc_type", "uniform")
    cfg.update(generalist=False, enc_emb=ctx["enc_emb"], enc_type=enc_type, contextflow=ctx["contextflow"])
    model = cfa.create_model(cfg, ds, MM, contexts=ctx["contexts"])
    model.load_state_dict(params, strict=True)
    model = model.to(DEV).eval()
    rep = 4096 // inp["x"].shape[0]
    tile = lambda t: t.repeat(rep, *([1] * (t.dim() - 1)))
    set_noise(model, tile(inp["u"]), [tile(e) for e in inp["eps"]])
    encs = [m for m in model.modules() if isinstance(m, cfa.layers.UniformCatDequantization)]
    assert len(encs) == len(inp["cnoise"])
    for e, c in zip(encs, inp["cnoise"]):
        e.fixed_noise = tile(c).to(DEV)
    z, logp = model(tile(inp["x"]).to(DEV), tile(inp["context"]).to(DEV))
    ref = tile(inp["logp"])
    tol = max(BPD_TOL, 1e-5 * bpd(inp["logp"], name).abs().max().item())
    assert (bpd(logp.cpu(), name) - bpd(ref, name)).abs().max().item() < tol
    assert (z.cpu() - tile(inp["z"])).abs().max().item() < 2e-3 * max(1.0, inp["z"].abs().max().item())
