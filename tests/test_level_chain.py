"""Level form of the evaluation flow step (cf_flow_step_fwd_level): the n <= 4 steps of one resolution level in ONE launch, z in
LDS from step to step.  It runs the same arithmetic in the same order as n launches of the saturating-batch kernel of the shape, so
every comparison here is BITWISE: z, and a running log-det that starts from non-zero values.  (run with -m gpu)"""
import ctypes

import pytest
import torch

DEV = "cuda:0"
CF_ERR_UNSUPPORTED = -2
# (C, H, W), batch, debug variant of the saturating-batch geometry (kDebugKernel in csrc/cf_step.hip: 4 = k_flow_step_small in the
# Winograd form, 6 = F(2x4) at 8x8 / 4x4).  3 samples at 16x16: three workgroups; 9 at 8x8: 4 samples per workgroup, a ragged
# last one of 1; 19 at 4x4: 8 per workgroup, a ragged last one of 3.  (8, 16, 16) stages its Winograd weights in LDS per step.
CASES = [((16, 16, 16), 3, 4), ((8, 16, 16), 3, 4), ((32, 8, 8), 9, 6), ((64, 4, 4), 19, 6)]


@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


_tables = {}


def tables(L, shape):
    """Four packed step tables of `shape` with seeded, non-trivial parameters (made once per shape, never written again)."""
    from contextflow_amd.layers import _hip
    if shape in _tables:
        return _tables[shape]
    C, H, W = shape
    f, pp = _hip.f32, _hip.p
    out = []
    for i in range(4):
        torch.manual_seed(1000 * C + i)
        conv, act, cpl = L.Conv1x1(shape), L.ActNorm(shape), L.Coupling(C, kernel_size=(3, 3), padding=(1, 1))
        with torch.no_grad():
            conv.NN.add_(0.1 * torch.randn(C, C))
            act.NN_t.copy_(0.3 * torch.randn(C)); act.NN_logs.copy_(0.2 * torch.randn(C))
            for p in cpl.parameters():          # (the reference initialises the last 1x1 with zeros: the affine map would be the identity)
                p.add_(0.05 * torch.randn_like(p))
        for m in (conv, act, cpl):
            m.to(DEV)
        ws = torch.empty(_hip.lib().cf_flow_step_ws_bytes(C, H, W), device=DEV, dtype=torch.uint8)
        c1, c2, c3 = cpl.NN[0], cpl.NN[2], cpl.NN[4]
        _hip.call("cf_flow_step_prepare", pp(f(conv.NN.detach())), pp(f(act.NN_t.detach())), pp(f(act.NN_logs.detach())),
                  pp(f(c1.weight.detach())), pp(f(c1.bias.detach())), pp(f(c2.weight.detach())), pp(f(c2.bias.detach())),
                  pp(f(c3.weight.detach())), pp(f(c3.bias.detach())), pp(ws), C, H, W, _hip.stream())
        out.append(ws)
    torch.cuda.synchronize()
    _tables[shape] = out
    return out


def debug_step(x, xbs, ws, ldj, shape, squeeze, variant):
    """One launch of the debug entry's kernel variant (no dumps); adds to ldj in place, returns z."""
    from contextflow_amd.layers import _hip
    fn = _hip.lib().cf_flow_step_fwd_debug
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    C, H, W = shape
    B = x.shape[0]
    z = torch.full((B, C, H, W), float("nan"), device=DEV)
    _hip.check(fn(_hip.p(x), _hip.p(z), _hip.p(ldj), _hip.p(ws), B, C, H, W, xbs, int(squeeze), None, variant << 16, _hip.stream()),
               "cf_flow_step_fwd_debug")
    return z


def level(x, xbs, tabs, ldj, shape, squeeze, form):
    from contextflow_amd.layers import _hip
    C, H, W = shape
    B = x.shape[0]
    z = torch.full((B, C, H, W), float("nan"), device=DEV)
    rc = _hip.lib().cf_flow_step_fwd_level(_hip.p(x), _hip.p(z), _hip.p(ldj), _hip.ptr_array(tabs), len(tabs), B, C, H, W, xbs, int(squeeze),
                                           form, _hip.stream())
    return rc, z


@pytest.mark.gpu
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("squeeze", [False, True])
@pytest.mark.parametrize("shape,B,variant", CASES)
def test_level_launch_equals_single_launches_bitwise(L, shape, B, variant, squeeze, strided):
    """form = 1 with n = 1, 2, 4 against n launches of the debug entry's variant of the same geometry: z and a pre-seeded, non-zero
    running log-det, bit for bit - with and without the squeeze folded into the first step, with a dense x and with a batch stride
    larger than C H W (the channel slice behind a SplitPrior)."""
    C, H, W = shape
    tabs = tables(L, shape)
    torch.manual_seed(7 * C + B)
    N = C * H * W
    xbs = 2 * N if strided else N
    buf = torch.randn(B, xbs, device=DEV)
    # squeeze: x is the (B, C/4, 2H, 2W) tensor in front of the Squeeze; either way the sample is the first N floats of its row
    x = buf[:, :N].view(B, C // 4, 2 * H, 2 * W) if squeeze else buf[:, :N].view(B, C, H, W)
    ldj0 = torch.randn(B, device=DEV) + 3.0
    for n in (1, 2, 4):
        ldj_ref = ldj0.clone()
        z_ref = debug_step(x, xbs, tabs[0], ldj_ref, shape, squeeze, variant)
        for ws in tabs[1:n]:
            z_ref = debug_step(z_ref, N, ws, ldj_ref, shape, False, variant)
        ldj = ldj0.clone()
        rc, z = level(x, xbs, tabs[:n], ldj, shape, squeeze, 1)
        torch.cuda.synchronize()
        assert rc == 0
        assert not torch.isnan(z_ref).any() and not torch.equal(ldj_ref, ldj0)
        assert torch.equal(z, z_ref), (n, (z - z_ref).abs().max().item())
        assert torch.equal(ldj, ldj_ref), (n, (ldj - ldj_ref).abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("shape,B,variant", CASES)
def test_form_0_below_the_minimum_launches_nothing(L, shape, B, variant):
    """form = 0 is the production dispatch: below cf_flow_step_level_min_batch it returns the not-a-level code and neither z nor
    the log-det is touched; the minimum is the threshold at which cf_flow_step_fwd takes the saturating-batch kernel."""
    from contextflow_amd.layers import _hip
    C, H, W = shape
    lib = _hip.lib()
    minb = lib.cf_flow_step_level_min_batch(C, H, W)
    assert minb == {256: lib.cf_flow_step_chain_max_batch(C, H, W) + 1, 64: 2048, 16: 2048}[H * W]
    assert B < minb
    x = torch.randn(B, C, H, W, device=DEV)
    ldj = torch.full((B,), 5.0, device=DEV)
    rc, z = level(x, C * H * W, tables(L, shape), ldj, shape, False, 0)
    torch.cuda.synchronize()
    assert rc == CF_ERR_UNSUPPORTED and b"not a level case" in lib.cf_last_error()
    assert torch.isnan(z).all() and torch.equal(ldj, torch.full((B,), 5.0, device=DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("name,records", [("cifar10", [(16, 256)] * 4 + [(32, 64)] * 4 + [(64, 16)] * 4), ("mnist", [(8, 256)] * 2 + [(32, 64)] * 2)])
def test_models_at_2051_samples(L, name, records):
    """The evaluation forward at 2 051 samples (above every level minimum; ragged last workgroups at 8x8 and 4x4): z and log p are
    bitwise the same with step_events unset, with step_events set, and with the level path disabled (LEVEL_STEPS empty: one launch
    per step).  With events set a level launch leaves one record per step: the first carries the launch, the others are empty."""
    from tests.gpu_util import build_model, set_noise
    from tests.helpers import load_e2e, e2e_inputs
    ops, _, M, params, fx = load_e2e(name)
    x, u, eps = e2e_inputs(name, fx)
    B = 2051
    rep = -(-B // x.shape[0])
    tile = lambda t: t.repeat(rep, *([1] * (t.dim() - 1)))[:B]
    model = build_model(name, params)
    model.auto_graph = False
    set_noise(model, None if u is None else tile(u), [tile(e) for e in eps])
    xin = tile(x).to(DEV)

    def run(events, levels):
        model.step_events = [] if events else None
        if not levels:
            model.LEVEL_STEPS = frozenset()
        try:
            with torch.no_grad():
                z, logp = model(xin)
            torch.cuda.synchronize()
            return z.clone(), logp.clone(), model.step_events
        finally:
            model.step_events = None
            model.__dict__.pop("LEVEL_STEPS", None)

    z0, lp0, _ = run(False, True)
    z1, lp1, ev = run(True, True)
    z2, lp2, ev2 = run(True, False)
    assert torch.isfinite(lp0).all()
    assert torch.equal(z0, z1) and torch.equal(lp0, lp1)
    assert torch.equal(z0, z2) and torch.equal(lp0, lp2)
    assert [(e[2], e[3], e[4]) for e in ev] == [(B, c, hw) for c, hw in records]
    assert [(e[2], e[3], e[4]) for e in ev2] == [(B, c, hw) for c, hw in records]
    # per level (runs of one shape): one record with the launch's two events, the rest with its end event twice
    from contextflow_amd.layers.flowsequential import FlowSequential
    i = 0
    while i < len(ev):
        j = i
        while j < len(ev) and ev[j][2:] == ev[i][2:]:
            j += 1
        if (ev[i][3], int(ev[i][4] ** 0.5), int(ev[i][4] ** 0.5)) in FlowSequential.LEVEL_STEPS:
            assert ev[i][0] is not ev[i][1]
            assert all(e[0] is e[1] and e[1] is ev[i][1] for e in ev[i + 1:j])
        i = j
    assert all(e[0] is not e[1] for e in ev2)
