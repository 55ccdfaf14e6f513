"""The sampling direction (`FlowSequential.inverse` / `sample`) against the fp64 flow at every level.

The exact answer of an inverse is free: run the fp64 oracle FORWARD with a trace (x -> z) and the trace itself is the
inverse of z, layer by layer, split-off halves included (oracle.flow_oracle.inverse_problem).  Nothing here inverts in fp64
on the GPU side of a comparison.

CPU (unmarked): the fp64 round trip of `flow_inverse`, and the floors the GPU bars rest on - what the REFERENCE's fp32
arithmetic (direct conditioner and its Winograd restatement) loses on one step in every parameter regime and on the whole
chain with default parameters.  The whole chain under the stress / extreme parameters is ill-conditioned in the reference's
own arithmetic (sampling section), so those regimes are held per step.

GPU (-m gpu): cf_flow_step_inv per geometry at 4099 / 4101 samples, batch-strided z, every fused step of the fixtures in
the three regimes, the whole cifar10 / mnist chains, an exact pixel cycle at 2053 samples, cf_gmm_sample, the direct form
of the conditioner in one child process, and `sample` at the benchmark batch.  Activations: 1e-5 of the tensor's scale
against fp64 - the bar of tests/test_gpu_parity.py.  Measured values: profiles/sampling_accuracy.md."""
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import flow_oracle as fo
from oracle.winograd import coupling_net_winograd
from tests.helpers import load_e2e, e2e_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ACT_TOL = 1e-5                    # activations against fp64, of the tensor's scale (tests/test_gpu_parity.py)
STEP_FLOOR = 2e-6                 # reference fp32 arithmetic, one step, every regime (measured worst 1.01e-6)
CHAIN_FLOOR = 2.5e-6              # reference fp32 arithmetic, whole chain, default parameters (measured 1.2e-6 / 7.1e-7)
PIXEL_FLOOR = 1.0 / 256           # ... in grey levels in front of the floor() (measured 5.6e-4 / 2.4e-4)
CYCLE_MARGIN = 1.0 / 64           # the exact-cycle test keeps x + u this far from the integers
CYCLE_B = 2048 + 5
REGIMES = [None, "stress", "extreme"]
FORMS = {"direct": fo.coupling_net, "winograd": coupling_net_winograd}


def scale_of(ref):
    return max(1.0, ref.abs().max().item())


def err_of(got, ref):
    """max |got - ref| in units of the reference's scale (the `close` of tests/test_gpu_parity.py, as a number)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return (got - ref).abs().max().item() / scale_of(ref)


def f64(params):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in params.items()}


def f32(params):
    return {k: (v.float() if v.is_floating_point() else v) for k, v in params.items()}


def traced(ops, params, x, u, eps):
    """fp64 forward with a trace -> (z, halves, inputs) in fp64 (oracle.flow_oracle.inverse_problem)."""
    tr = []
    x = x.double()
    fo.flow_forward(ops, f64(params), x, None if u is None else u.double(), [e.double() for e in eps], trace=tr)
    return fo.inverse_problem(ops, x, tr)


@functools.lru_cache(maxsize=None)
def fixture_problem(name, tag=None):
    """(ops, params, z, halves, inputs) of a committed e2e fixture: its samples and captured noise through the fp64 oracle."""
    ops, _, _, params, fx = load_e2e(name, tag)
    x, u, eps = e2e_inputs(name, fx)
    return (ops, params) + traced(ops, params, x, u, eps)


def fused_steps(ops):
    """[(index of the conv1x1, a Squeeze((2,2)) sits in front)] of every Conv1x1 -> ActNorm -> Coupling group."""
    out = []
    for i in range(len(ops) - 2):
        if (ops[i][0], ops[i + 1][0], ops[i + 2][0]) == ("conv1x1", "actnorm", "coupling"):
            out.append((i, i > 0 and ops[i - 1][0] == "squeeze" and tuple(ops[i - 1][2]) == (2, 2)))
    return out


def op_index(ops, kind):
    return next(i for i, o in enumerate(ops) if o[0] == kind)


def with_form(form, fn):
    """Run fn() with the oracle's conditioner in the given form (the Winograd restatement is fp32 only)."""
    keep = fo.coupling_net
    try:
        fo.coupling_net = FORMS[form]
        return fn()
    finally:
        fo.coupling_net = keep


def cycle_inputs(name):
    """Inputs of the exact pixel cycle: uint8 pixels, dequantisation noise in [1/64, 63/64], Augment noise."""
    C, H, W = fo.CONFIGS[name][0]
    g = torch.Generator().manual_seed(2053 + C)
    x = torch.randint(0, 256, (CYCLE_B, C, H, W), generator=g).float()
    u = CYCLE_MARGIN + (1.0 - 2.0 * CYCLE_MARGIN) * torch.rand(CYCLE_B, C, H, W, generator=g)
    eps = [torch.randn(CYCLE_B, 1, H, W, generator=g)]
    assert u.min().item() >= CYCLE_MARGIN and u.max().item() <= 1.0 - CYCLE_MARGIN
    return x, u, eps


# ---- CPU: the oracle's inverse and the reference-arithmetic floors --------------------------------------------------------
@pytest.mark.parametrize("name", ["cifar10", "mnist", "smap"])
def test_fp64_round_trip_recovers_the_trace(name):
    """flow_inverse in fp64 walks back through the forward trace: every layer input to 1e-9 of its scale (the fp64 bar of
    tests/test_oracle_golden.py), the pixels exactly."""
    ops, params, z, halves, inputs = fixture_problem(name)
    back = []
    x = fo.flow_inverse(ops, f64(params), z, halves, trace=back)
    assert x.dtype == torch.float64 and len(back) == len(ops)
    worst = 0.0
    for kind, idx, got in back:
        i = next(j for j, o in enumerate(ops) if o[1] == idx)
        e = err_of(got, inputs[i])
        worst = max(worst, e)
        assert e <= 1e-9, (kind, idx, e)
    if name == "smap":
        print("%s fp64 round trip: worst layer input %.2e of scale" % (name, worst))
        return
    a = op_index(ops, "augment")
    logit = fo.flow_inverse(ops, f64(params), z, halves, stop="augment")
    e = err_of(logit, inputs[a + 1])
    print("%s fp64 round trip: logit space %.2e of scale %.2f, worst layer input %.2e" % (name, e, scale_of(inputs[a + 1]), worst))
    assert e <= 1e-9
    assert torch.equal(x, inputs[0]) and torch.equal(x, x.floor())
    assert len(halves) == sum(o[0] == "split" for o in ops)
    # the same walk without the halves has no answer, and the layer-only entry point still refuses a split
    if halves:
        with pytest.raises(ValueError):
            fo.flow_inverse(ops, f64(params), z)
        with pytest.raises(ValueError):
            fo.flow_inverse_layers(ops[a + 1:], f64(params), z)


def step_inverse_fp32(ops, p32, i, z):
    pre = "%d." % ops[i][1]
    h = fo.coupling_inv(z, p32, "%d." % ops[i + 2][1], ops[i + 2][4])
    h = fo.actnorm_inv(h, p32["%d.NN_t" % ops[i + 1][1]], p32["%d.NN_logs" % ops[i + 1][1]])
    return fo.conv1x1_inv(h, p32[pre + "NN"])


def step_floors(name, tag):
    """{(C, H): {form: worst error of scale}} of the fp32 oracle inverse of every fused step, fed the fp64 trace."""
    ops, params, z, halves, inputs = fixture_problem(name, tag)
    p32 = f32(params)
    out = {}
    for i, _ in fused_steps(ops):
        geo = tuple(inputs[i].shape[1:3])
        for form in FORMS:
            got = with_form(form, lambda: step_inverse_fp32(ops, p32, i, inputs[i + 3].float()))
            assert got.dtype == torch.float32
            d = out.setdefault(geo, {})
            d[form] = max(d.get(form, 0.0), err_of(got, inputs[i]))
    return out


@pytest.mark.parametrize("tag", REGIMES)
@pytest.mark.parametrize("name", ["cifar10", "mnist"])
def test_reference_floor_of_one_inverse_step(name, tag):
    """Coupling^-1, ActNorm^-1, Conv1x1^-1 in the reference's fp32 arithmetic, on the fp64 trace's step outputs rounded to
    fp32, against the trace's step inputs: at most 2e-6 of scale in every regime and both forms of the conditioner.  One step
    is well-conditioned where the chain is not - the fact the GPU bar of 1e-5 rests on."""
    floors = step_floors(name, tag)
    assert len(floors) == {"cifar10": 3, "mnist": 2}[name]
    for geo, d in sorted(floors.items()):
        print("%s %s step C=%d H=%d: fp32 reference inverse  direct %.2e  winograd %.2e  of scale" % (name, tag, geo[0], geo[1], d["direct"], d["winograd"]))
        assert max(d.values()) <= STEP_FLOOR, (geo, d)


def chain_floor(ops, params, z, halves, inputs, form):
    """(logit-space error of scale, error in grey levels in front of the floor, pixels wrong) of the fp32 oracle chain."""
    p32 = f32(params)
    z32, h32 = z.float(), [h.float() for h in halves]
    a = op_index(ops, "augment")
    logit = with_form(form, lambda: fo.flow_inverse(ops, p32, z32, h32, stop="augment"))
    pre = with_form(form, lambda: fo.flow_inverse(ops, p32, z32, h32, stop="dequant"))
    assert logit.dtype == torch.float32
    grey = (pre.double() - inputs[1]).abs().max().item()
    return err_of(logit, inputs[a + 1]), grey, int((pre.floor().double() != inputs[0]).sum())


@pytest.mark.parametrize("name", ["cifar10", "mnist"])
def test_reference_floor_of_the_chain(name):
    """The whole reverse chain in the reference's fp32 arithmetic on the default fixtures (z and the split halves of the fp64
    trace rounded to fp32): logit space within 2.5e-6 of scale, the pixels in front of the floor within 1/256 grey level."""
    prob = fixture_problem(name)
    for form in FORMS:
        e, grey, wrong = chain_floor(*prob, form)
        print("%s chain, fp32 reference inverse, %s: logit space %.2e of scale %.2f, %.2e grey levels before the floor, %d pixels wrong"
              % (name, form, e, scale_of(prob[4][op_index(prob[0], "augment") + 1]), grey, wrong))
        assert e <= CHAIN_FLOOR and grey <= PIXEL_FLOOR


@pytest.mark.parametrize("name", ["cifar10", "mnist"])
def test_reference_floor_on_the_inputs_of_the_pixel_cycle(name):
    """The first 16 rows of the exact-cycle test's inputs: the reference arithmetic lands within 1/256 grey level of
    x + u, four times inside the 1/64 that the noise keeps x + u away from the integers - so floor() returns x exactly, and
    the GPU test may demand every pixel."""
    ops, _, _, params, _ = load_e2e(name)
    x, u, eps = cycle_inputs(name)
    n = 16
    z, halves, inputs = traced(ops, params, x[:n], u[:n], [e[:n] for e in eps])
    for form in FORMS:
        e, grey, wrong = chain_floor(ops, params, z, halves, inputs, form)
        print("%s cycle inputs, fp32 reference inverse, %s: logit space %.2e of scale, %.2e grey levels before the floor (margin %.2e)"
              % (name, form, e, grey, CYCLE_MARGIN))
        assert grey <= PIXEL_FLOOR and PIXEL_FLOOR * 4 <= CYCLE_MARGIN and wrong == 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


def conditioner_form(C, H, B):
    """'direct' | 'winograd': the form cf_flow_step_inv runs its 3x3 in, read from the dispatch's own multiply-add count,
    and checked against the process-wide switch."""
    from contextflow_amd.layers import _hip
    macs = _hip.lib().cf_flow_step_macs(B, C, H, H, 3)
    form = {40: "direct", 20: "winograd"}[macs // (C * C * H * H)]
    assert form == ("direct" if os.environ.get("CONTEXTFLOW_DIRECT_CONV", "")[:1] == "1" else "winograd")
    return form


def step_modules(L, C, H):
    """The parameters of test_winograd_step_kernel_against_the_oracle (tests/test_gpu_parity.py)."""
    torch.manual_seed(C * 1000 + 7)
    conv, act, cpl = L.Conv1x1((C, H, H)), L.ActNorm((C, H, H)), L.Coupling(C, kernel_size=(3, 3), padding=(1, 1))
    with torch.no_grad():
        conv.NN.add_(0.1 * torch.randn(C, C))
        act.NN_t.copy_(0.3 * torch.randn(C)); act.NN_logs.copy_(0.2 * torch.randn(C)); act.initialized.fill_(1)
    act._init_done = True
    return conv, act, cpl


def step_flow(L, conv, act, cpl, C, H, squeeze):
    import contextflow_amd as cfa
    dist = L.GaussianMixtureDistribution(size=(C, H, H), mixtures=2, components=8)
    mods = ([L.Squeeze((2, 2))] if squeeze else []) + [conv, act, cpl]
    return cfa.layers.FlowSequential(dist, *mods).to(DEV)


def run_inverse(flow, z, B, C, HW):
    """flow.inverse(z) with the launch record: exactly one cf_flow_step_inv of (B, C, HW) - the fused kernel, not the chain."""
    flow.inv_events = []
    try:
        out = flow.inverse(z)
        torch.cuda.synchronize()
        launches = [(e[2], e[3], e[4]) for e in flow.inv_events]
    finally:
        flow.inv_events = None
    assert launches == [(B, C, HW)], launches
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("squeeze", [False, True])
@pytest.mark.parametrize("C,H", [(8, 16), (16, 16), (32, 8), (64, 4)])
def test_inverse_step_at_production_batch(L, C, H, squeeze):
    """cf_flow_step_inv through FlowSequential.inverse at 4099 and 4101 samples (the last workgroup holds 3 / 1 of 4, 3 / 5
    of 16, 1 of 1): x random, z = the fp64 oracle forward of the step, so the exact answer is x.  1e-5 of scale."""
    conv, act, cpl = step_modules(L, C, H)
    Bmax = 4101
    x = torch.randn(Bmax, C, H, H)
    p = {"0." + k: v.detach().double() for k, v in cpl.state_dict().items()}
    y, _ = fo.conv1x1_fwd(x.double(), conv.NN.detach().double())
    y, _ = fo.actnorm_fwd(y, act.NN_t.detach().double(), act.NN_logs.detach().double())
    z, _ = fo.coupling_fwd(y, p, "0.", (1, 1))
    # the reference-arithmetic floor on the same problem (256 rows of it)
    p32 = {k: v.float() for k, v in p.items()}
    ref32 = fo.conv1x1_inv(fo.actnorm_inv(fo.coupling_inv(z[:256].float(), p32, "0.", (1, 1)), act.NN_t.detach(), act.NN_logs.detach()),
                           conv.NN.detach())
    floor = err_of(ref32, x[:256])
    flow = step_flow(L, conv, act, cpl, C, H, squeeze)
    form = conditioner_form(C, H, Bmax)
    for B in (4099, 4101):
        want = fo.squeeze_inv(x[:B], (2, 2)) if squeeze else x[:B]
        got = run_inverse(flow, z[:B].float().to(DEV), B, C, H * H)
        assert tuple(got.shape) == tuple(want.shape)
        e = err_of(got, want)
        tail = err_of(got[B - 16:], want[B - 16:]) * scale_of(want[B - 16:]) / scale_of(want)
        print("inverse step C=%d H=%d squeeze=%d B=%d %s: %.2e of scale (last 16 rows %.2e; fp32 reference floor %.2e; bar %.0e)"
              % (C, H, squeeze, B, form, e, tail, floor, ACT_TOL))
        assert e <= ACT_TOL, (B, e)


@pytest.mark.gpu
@pytest.mark.parametrize("C,H", [(8, 16), (16, 16), (32, 8), (64, 4)])
def test_inverse_step_reads_a_batch_strided_z(L, C, H):
    """z as a channel slice of a wider tensor (batch stride > C H W, first and last channels of it): bitwise the result on
    the contiguous copy.  The kernel reads z twice through its batch stride - once for the conditioner, once for z1."""
    from contextflow_amd.layers import _hip
    conv, act, cpl = step_modules(L, C, H)
    for squeeze in (False, True):
        flow = step_flow(L, conv, act, cpl, C, H, squeeze)
        for B in (4099, 5):
            g = torch.Generator().manual_seed(B + C)
            z = torch.randn(B, C, H, H, generator=g).to(DEV)
            want = run_inverse(flow, z, B, C, H * H)
            for extra, front in ((4, False), (C, True)):
                wide = torch.randn(B, C + extra, H, H, generator=g).to(DEV) * 50.0
                zs = wide[:, extra:] if front else wide[:, :C]
                zs.copy_(z)
                v, zbs = _hip.bview(zs)
                assert zbs == (C + extra) * H * H and v.data_ptr() == zs.data_ptr() and not zs.is_contiguous()
                got = run_inverse(flow, zs, B, C, H * H)
                same = torch.equal(got, want)
                print("strided z C=%d H=%d squeeze=%d B=%d batch stride %d (dense %d) offset %d: bitwise %s"
                      % (C, H, squeeze, B, zbs, C * H * H, zs.data_ptr() - wide.data_ptr(), same))
                assert same, (squeeze, B, extra, (got - want).abs().max().item())


def tile_rows(t, B):
    n0 = t.shape[0]
    return t.repeat((B + n0 - 1) // n0, *([1] * (t.dim() - 1)))[:B]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", REGIMES)
@pytest.mark.parametrize("name", ["cifar10", "mnist"])
def test_every_fused_step_of_the_fixtures(L, name, tag):
    """The model's own _inverse_step on the fp64 trace's step outputs, tiled to a ragged batch above 2048, against the
    trace's step inputs - default, stress and extreme parameters (trained-like log-scales, the C = 64 inverse).  1e-5 of
    scale; the reference's fp32 arithmetic sits at 1e-6 on the same tensors (test_reference_floor_of_one_inverse_step)."""
    from tests.gpu_util import build_model
    import contextflow_amd as cfa
    ops, params, z, halves, inputs = fixture_problem(name, tag)
    floors = step_floors(name, tag)
    model = build_model(name, params)
    mods = model.sequence_modules
    n0 = z.shape[0]
    B = n0 * (2048 // n0 + 1) - 3
    assert B >= 2048 and B % 16 != 0
    steps = fused_steps(ops)
    assert len(steps) == {"cifar10": 12, "mnist": 4}[name]
    for i, sq in steps:
        conv, act, cpl = mods[i], mods[i + 1], mods[i + 2]
        assert isinstance(conv, cfa.layers.Conv1x1) and isinstance(act, cfa.layers.ActNorm) and isinstance(cpl, cfa.layers.Coupling)
        C, H = inputs[i].shape[1:3]
        form = conditioner_form(C, H, B)
        from contextflow_amd.layers.inverse import _inverse_step
        model.inv_events = []
        try:
            got = _inverse_step(model, tile_rows(inputs[i + 3].float(), B).to(DEV), conv, act, cpl, unsqueeze=sq)
            torch.cuda.synchronize()
            assert [(e[2], e[3], e[4]) for e in model.inv_events] == [(B, C, H * H)]
        finally:
            model.inv_events = None
        want = tile_rows(inputs[i - 1] if sq else inputs[i], B)
        e = err_of(got, want)
        print("%s %s step %d C=%d H=%d unsqueeze=%d B=%d %s: %.2e of scale %.1f (fp32 reference floor %.2e; bar %.0e)"
              % (name, tag, ops[i][1], C, H, sq, B, form, e, scale_of(want), floors[(C, H)][form], ACT_TOL))
        assert e <= ACT_TOL, (ops[i][1], e)
        gc = got.cpu()
        assert torch.equal(gc, gc[torch.arange(B) % n0])           # every copy of a row, the tail workgroup's too, gives the same bits


def flow_part(model, ops):
    """The modules behind the Augment as a FlowSequential of their own (shared module objects): its inverse ends in logit
    space, the Augment noise channel still attached."""
    import contextflow_amd as cfa
    a = op_index(ops, "augment")
    assert isinstance(model.sequence_modules[a], cfa.layers.Augment)
    sub = cfa.layers.FlowSequential(model.dist, *model.sequence_modules[a + 1:])
    return sub, a


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cifar10", "mnist"])
def test_whole_chain_against_the_fp64_trace(L, name):
    """z and the recorded split halves of the fp64 trace through the flow part of the model, fused and layer by layer, at
    the fixture's batch and tiled to 4099 rows, against the trace's logit-space tensor: 1e-5 of scale.  The cifar10 chain
    holds two SplitPrior.reverse, the C = 16 and C = 64 inverse kernels and the folded un-squeeze."""
    from tests.gpu_util import build_model, set_split_draws
    ops, params, z, halves, inputs = fixture_problem(name)
    model = build_model(name, params)
    sub, a = flow_part(model, ops)
    want = inputs[a + 1]
    n0, Bbig = z.shape[0], 4096 + 3
    floor = max(chain_floor(ops, params, z, halves, inputs, form)[0] for form in FORMS)
    n_steps = len(fused_steps(ops))
    out = {}
    for fused in (True, False):
        sub.fused = fused
        for B in (n0, Bbig):
            sub.inv_events = []
            try:
                with set_split_draws(model, [tile_rows(h.float(), B) for h in halves]):
                    got = sub.inverse(tile_rows(z.float(), B).to(DEV))
                torch.cuda.synchronize()
                assert len(sub.inv_events) == (n_steps if fused else 0)
            finally:
                sub.inv_events = None
            e = err_of(got, tile_rows(want, B))
            print("%s chain %s B=%d: logit space %.2e of scale %.2f (fp32 reference floor %.2e; bar %.0e)"
                  % (name, "fused" if fused else "layers", B, e, scale_of(want), floor, ACT_TOL))
            assert e <= ACT_TOL, (fused, B, e)
            out[fused, B] = got.cpu()
        # rows of the large run against the same rows run alone: both within 1e-5 of the exact answer
        big, small = out[fused, Bbig], out[fused, n0]
        for lo in (0, Bbig - Bbig % n0 - n0):
            d = (big[lo:lo + n0] - small).abs().max().item() / scale_of(want)
            print("%s chain %s rows %d..%d of %d against the %d rows alone: %.2e of scale, bitwise %s"
                  % (name, "fused" if fused else "layers", lo, lo + n0, Bbig, n0, d, torch.equal(big[lo:lo + n0], small)))
            assert d <= 2 * ACT_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cifar10", "mnist"])
def test_exact_pixel_cycle_at_a_ragged_batch(L, name):
    """2053 random uint8 images, dequantisation noise in [1/64, 63/64]: z, the Augment noise and the split halves from the
    fp64 oracle trace, then model.inverse(z), fused, cf_postprocess_inv included, returns EVERY pixel of EVERY sample.  The
    margin is a condition, not a tolerance: the reference's fp32 arithmetic is within 1/256 grey level in front of the
    floor on these inputs (test_reference_floor_on_the_inputs_of_the_pixel_cycle), a kernel at the 1e-5 bar likewise."""
    from tests.gpu_util import build_model, set_split_draws
    ops, _, _, params, _ = load_e2e(name)
    x, u, eps = cycle_inputs(name)
    z, halves, inputs = traced(ops, params, x, u, eps)
    model = build_model(name, params)
    assert model.fused
    zd = z.float().to(DEV)
    with set_split_draws(model, [h.float() for h in halves]):
        got = model.inverse(zd)
        sub, a = flow_part(model, ops)
        logit = sub.inverse(zd)
    e = err_of(logit, inputs[a + 1])
    wrong = got.cpu() != x
    print("%s pixel cycle B=%d: %d of %d pixels wrong in %d samples; logit space %.2e of scale"
          % (name, CYCLE_B, int(wrong.sum()), wrong.numel(), int(wrong.flatten(1).any(1).sum()), e))
    assert tuple(got.shape) == tuple(x.shape) and got.dtype == torch.float32
    assert not wrong.any()


def gmm_sample_call(mG, sG, rows, eps, out, N, D):
    from contextflow_amd.layers import _hip
    _hip.call("cf_gmm_sample", _hip.p(mG), _hip.p(sG), _hip.p(rows), _hip.p(eps), _hip.p(out), N, D, _hip.stream())
    torch.cuda.synchronize()


def gmm_formula(mG, sG, rows, eps):
    """mG[row] + softplus(sG[row]) * eps in fp64 (gaussian.py:163-169)."""
    r = rows.cpu()
    return mG.cpu().double()[r] + F.softplus(sG.cpu().double()[r]) * eps.cpu().double()


def gmm_close(out, ref):
    return ((out.cpu().double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item() if ref.numel() else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("D", [2048, 768, 96, 7, 1])
def test_gmm_sample_kernels_against_the_formula(L, D):
    """cf_gmm_sample, the 16-byte kernel (D % 4 == 0, aligned pointers) and the scalar one (D = 7, 1, or any pointer 4 bytes
    off), N = 1, 3, 1001 and 0, rows that hit the first and the last of the M K parameter rows: 1e-6 of max(1, |out|) - a
    few fp32 ulp of the softplus times |eps| <= ~5.  Sentinels around the output catch a store outside it."""
    M, K = 3, 5
    g = torch.Generator().manual_seed(D)
    mG = (3.0 * torch.randn(M * K, D, generator=g)).to(DEV)
    sG = (8.0 * torch.rand(M * K, D, generator=g) - 4.0).to(DEV)           # softplus from 0.018 to 4.02
    worst = 0.0
    for N in (1, 3, 1001, 0):
        for first in ((0, M * K - 1) if N == 1 else (0,)):
            rows = torch.randint(0, M * K, (max(N, 1),), generator=g)
            rows[0], rows[-1] = first, (M * K - 1 if N > 1 else first)
            rows = rows[:N].to(DEV) if N else rows.to(DEV)
            eps = torch.randn(N, D, generator=g).to(DEV)
            ref = gmm_formula(mG, sG, rows[:N], eps)
            pad = 8
            buf = torch.full((N * D + 2 * pad,), 12345.0, device=DEV)
            out = buf[pad:pad + N * D].view(N, D)                          # 32 bytes in: still 16-byte aligned
            gmm_sample_call(mG, sG, rows, eps, out, N, D)
            assert torch.all(buf[:pad] == 12345.0) and torch.all(buf[pad + N * D:] == 12345.0)
            e = gmm_close(out, ref)
            worst = max(worst, e)
            assert e <= 1e-6, (N, D, e)
            if N == 0:
                continue
            # every operand in turn 4 bytes off a 16-byte boundary: the scalar kernel, the same numbers
            for which in range(4):
                ops_ = [mG, sG, eps, None]
                buf2 = torch.full((N * D + 2 * pad + 1,), 12345.0, device=DEV)
                out2 = (buf2[pad + 1:pad + 1 + N * D] if which == 3 else buf2[pad:pad + N * D]).view(N, D)
                if which < 3:
                    src = ops_[which]
                    shifted = torch.empty(src.numel() + 1, device=DEV)[1:].view(src.shape)
                    shifted.copy_(src)
                    assert shifted.data_ptr() % 16 == 4
                    ops_[which] = shifted
                else:
                    assert out2.data_ptr() % 16 == 4
                gmm_sample_call(ops_[0], ops_[1], rows, ops_[2], out2, N, D)
                lo = pad + (1 if which == 3 else 0)
                assert torch.all(buf2[:lo] == 12345.0) and torch.all(buf2[lo + N * D:] == 12345.0)
                assert gmm_close(out2, ref) <= 1e-6, (N, D, which)
                assert torch.equal(out2, out), (N, D, which)
    print("cf_gmm_sample D=%d: worst error %.2e of max(1, |out|) (bar 1e-06)" % (D, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("M,size", [(10, (8, 16, 16)), (1, (24, 2, 2)), (3, (7, 1, 1))])
def test_gmm_distribution_sample_against_the_formula(L, M, size):
    """GaussianMixtureDistribution.sample as a whole: under a seed its two draws (multinomial over the softmax of
    wG[m], then randn) are replayed in order and x must be mG[m, k] + softplus(sG[m, k]) eps with m = 1 (the reference
    hard-codes the class-mixture 1) or 0 for a single mixture; need_log_prob=False returns the same x."""
    K, n = 8, 777
    torch.manual_seed(M)
    dist = L.GaussianMixtureDistribution(size=size, mixtures=M, components=K).to(DEV)
    with torch.no_grad():
        dist.sG.copy_(4.0 * torch.rand_like(dist.sG) - 2.0)
        dist.mG.mul_(2.0)
    D = size[0] * size[1] * size[2]
    torch.manual_seed(31)
    x, lp = dist.sample(n)
    torch.manual_seed(31)
    x2, none = dist.sample(n, need_log_prob=False)
    torch.manual_seed(31)
    m = 1 if M > 1 else 0
    k = torch.multinomial(torch.softmax(dist.wG.detach()[m].float(), dim=-1), n, replacement=True)
    eps = torch.randn(n, D, device=DEV, dtype=torch.float32)
    assert tuple(x.shape) == (n,) + tuple(size) and tuple(lp.shape) == (n, M) and none is None
    assert torch.equal(x, x2)
    assert len(set(k.tolist())) > 1                                        # the draw uses several components
    ref = gmm_formula(dist.mG.detach().reshape(M * K, D), dist.sG.detach().reshape(M * K, D), m * K + k, eps)
    e = gmm_close(x.reshape(n, D), ref)
    print("GaussianMixtureDistribution.sample M=%d D=%d: %.2e of max(1, |x|) (bar 1e-06)" % (M, D, e))
    assert e <= 1e-6
    lp_ref = fo.gmm_logprob(x.cpu().double(), dist.mG.detach().cpu().double(), dist.sG.detach().cpu().double(), dist.wG.detach().cpu().double())
    assert ((lp.cpu().double() - lp_ref).abs() / lp_ref.abs().clamp_min(1.0)).max().item() <= 1e-5


@pytest.mark.gpu
def test_direct_form_of_the_conditioner_in_a_child_process():
    """CONTEXTFLOW_DIRECT_CONV=1 is read once per process: the per-geometry and the per-fixture-step tests above run once
    more in ONE fresh child, where they assert that the inverse dispatch reports the direct form.  The child runs under a
    time limit; if it does not exit 0 nothing further is started."""
    env = dict(os.environ, CONTEXTFLOW_DIRECT_CONV="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_sampling.py"), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           "-k", "test_inverse_step_at_production_batch or test_every_fused_step_of_the_fixtures"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if " direct: " in ln]
    print("\n".join(lines))
    print(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "")
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert len(lines) == 8 * 2 + 3 * 12 + 3 * 4 and not any(" winograd: " in ln for ln in r.stdout.splitlines())


BENCH_B = 16384


def bench_sample(seed):
    from tests.gpu_util import build_model
    ops, _, _, params, _ = load_e2e("cifar10")
    model = build_model("cifar10", params)
    torch.manual_seed(seed)
    a = model.sample(BENCH_B)
    torch.cuda.synchronize()
    return model, a


@pytest.mark.gpu
def test_sample_at_the_bench_batch(L):
    """model.sample(16384) of cifar10, the call bench.py times: shape, finite, integer valued; a second call under the same
    seed is bitwise the first (cached step tables, event ordering on a warm cache), another seed gives other pixels.  The
    range of the pixels is the test below."""
    model, a = bench_sample(7)
    torch.manual_seed(7)
    b = model.sample(BENCH_B)
    torch.manual_seed(8)
    c = model.sample(BENCH_B)
    torch.cuda.synchronize()
    assert tuple(a.shape) == (BENCH_B,) + tuple(fo.CONFIGS["cifar10"][0]) and a.dtype == torch.float32
    assert torch.isfinite(a).all() and torch.equal(a, a.floor())
    assert torch.equal(a, b) and not torch.equal(a, c)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_sample_at_the_bench_batch_stays_in_0_255(L, fused):
    """Every pixel of model.sample(16384) in [0, 255].

    The reverse chain alone does not give that: it ends in floor(256 (sigmoid(y) - a) / (1 - 2 a)), a = 1e-4, with no clamp
    (dequantize.py:19-20, normalize.py:36-40) - -1 for y < logit(a) = -9.21 and 256 for y > 9.21 - and a prior draw pushed
    through untrained couplings reaches those logits: with the parameters of the e2e_cifar10 fixture and seed 7, 307 052
    pixels of -1 and 293 875 of 256 in 50 331 648 (1.2 %), in every one of the 16 384 samples; the reference's own z -> x
    vectors hold both values (tests/golden/inverse_mnist.npz).  `sample` therefore projects into the data range
    (cf_postprocess_inv_clamped in the fused tail, cf_clamp behind the layer chain) and `inverse` stays the plain chain:
    under the same seed sample(B) is bitwise clamp(inverse(z), 0, 255) of the same draws, and the clamp has work to do."""
    from tests.gpu_util import build_model
    ops, _, _, params, _ = load_e2e("cifar10")
    model = build_model("cifar10", params)
    model.fused = fused
    torch.manual_seed(7)
    a = model.sample(BENCH_B)
    torch.manual_seed(7)
    z = model.dist.sample(BENCH_B, need_log_prob=False)[0]        # the draws of `sample`, in its order: the prior, then the split halves
    raw = model.inverse(z)
    torch.cuda.synchronize()
    lo, hi = int((raw < 0).sum()), int((raw > 255).sum())
    print("sample(16384) %s: min %.0f max %.0f mean %.2f; the reverse chain alone: min %.0f max %.0f, %d pixels below 0 and %d above 255 of %d"
          % ("fused" if fused else "layers", a.min().item(), a.max().item(), a.mean().item(), raw.min().item(), raw.max().item(), lo, hi, raw.numel()))
    assert tuple(a.shape) == (BENCH_B,) + tuple(fo.CONFIGS["cifar10"][0]) and torch.equal(a, a.floor())
    assert a.min().item() >= 0 and a.max().item() <= 255
    assert raw.min().item() == -1 and raw.max().item() == 256 and lo > 0 and hi > 0
    assert torch.equal(a, raw.clamp(0.0, 255.0))
