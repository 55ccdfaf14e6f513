"""The zero-skipping F(2x4, 3x3) kernel of the 4x4 level (contextflow_amd/csrc/cf_step_common.h: Geo::ZSKIP, G64z24): 16 samples
per workgroup on 8 waves, every column tile of 16 output tiles at ONE tile row, and a wave leaves out the vertical index whose two
patch rows reflect padding makes the same image row (xi = 0 at tile row 0, xi = 3 at tile row 1: d - d = +0 in every lane).
CPU: the h1 order of that geometry (bijection, LDS banks of the patch reads and of phase 1's stores) and the row coincidence the
skip rests on.  GPU: the kernel (debug variant 7) against the F(2x4) kernel it replaces (variant 6), bit for bit, at batches
around one workgroup; against the fp64 oracle; and an end-to-end log-density above the dispatch threshold with the kernel
switched on and off."""
import ctypes
import os

import pytest
import torch

from oracle import flow_oracle as fo
from tests.helpers import load_e2e, e2e_inputs

DEV = "cuda:0"
C, H, W = 64, 4, 4
HALF, HID, HW = C // 2, 2 * C, H * W
SPW, WAVES = 16, 8
PIX = SPW * HW                      # 256 pixels = 1 KB per plane row


# ---- the h1 order: a restatement of w24z_pix and of the lane maps of phases 1 and 2 ----------------------------------------
def w24z_pix(s, y, x, k):
    R = 2 * y + (x >> 1)
    return 32 * R + 16 * ((x ^ k) & 1) + ((s ^ (2 * R)) & 15)


def reflect(v, n):
    return -v if v < 0 else (2 * (n - 1) - v if v >= n else v)


R1 = {0: 0, 1: 1, 2: 2, 3: 1}        # B2^T row xi = d[r1] + sigma d[r2], sigma = -1 but at xi = 1
R2 = {0: 2, 1: 2, 2: 1, 3: 3}
PATCH_COL = [1, 0, 1, 2, 3, 2]       # image column of patch column c of the one tile of an image row (reflect(-1), 0..3, reflect(4))


def test_the_order_is_a_bijection_onto_the_hidden_planes():
    words = set()
    for row in range(HID):
        for s in range(SPW):
            for y in range(H):
                for x in range(W):
                    w = w24z_pix(s, y, x, row & 1)
                    assert 0 <= w < PIX
                    words.add(row * PIX + w)
    assert len(words) == HID * PIX and min(words) == 0 and max(words) == HID * PIX - 1


def test_every_patch_read_group_hits_32_banks():
    """A ds_read_b32 is served in two groups of 32 lanes on 32 banks.  Lane = 16 lg + l15: sample l15, k row lg of the k-step; the
    tile row is the wave's (column tile ct = wave & 1).  For each of the 4 x 6 patch elements, each k-step and each wave parity."""
    for ct in range(2):
        for a in range(4):
            y = reflect(2 * ct - 1 + a, H)
            for c in range(6):
                x = PATCH_COL[c]
                assert x == reflect(c - 1, W)
                for kstep in range(0, HID, 4):          # rows kstep + lg of the plane behind the y0 rows
                    for group in range(2):
                        banks = set()
                        for lane in range(32 * group, 32 * group + 32):
                            l15, lg = lane & 15, lane >> 4
                            word = (HALF + kstep + lg) * PIX + w24z_pix(l15, y, x, lg & 1)
                            banks.add(word % 32)
                        assert len(banks) == 32, (ct, a, c, kstep, group)


def test_phase_1_stores_hit_32_banks():
    """A 32-lane group of a phase-1 store: the wave's 32 pixels (two samples) at one plane row."""
    for wave in range(WAVES):
        for row in range(HID):
            banks = set()
            for li in range(32):
                pix = wave * 32 + li
                s, pin = pix // HW, pix % HW
                banks.add((row * PIX + w24z_pix(s, pin // W, pin % W, row & 1)) % 32)
            assert len(banks) == 32, (wave, row)


def test_the_skipped_rows_coincide():
    """xi = 0 at tile row 0 and xi = 3 at tile row 1 subtract one image row from itself; no other (xi, tile row) of a 4-row image
    does (the static_assert beside the kernel's skip checks the same two)."""
    zero = {(xi, ty) for xi in range(4) for ty in range(2)
            if xi != 1 and reflect(2 * ty - 1 + R1[xi], H) == reflect(2 * ty - 1 + R2[xi], H)}
    assert zero == {(0, 0), (3, 1)}


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


def step_variant(x, ws, ldj0, squeeze, variant):
    """cf_flow_step_fwd_debug without dumps: the kernel variant of the dispatch table (6 = F(2x4), 7 = ... zero-skipping), on a
    copy of the running log-det ldj0."""
    from contextflow_amd.layers import _hip
    fn = _hip.lib().cf_flow_step_fwd_debug
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    B = x.shape[0]
    z = torch.full((B, C, H, W), float("nan"), device=x.device)
    ldj = ldj0.clone()
    _hip.check(fn(_hip.p(x), _hip.p(z), _hip.p(ldj), _hip.p(ws), B, C, H, W, C * H * W, int(squeeze), None, variant << 16,
                  _hip.stream()), "cf_flow_step_fwd_debug")
    torch.cuda.synchronize()
    return z, ldj


def seeded_step(L, B):
    """The parameters and inputs of tests/test_winograd24.py's step test at C = 64, at a batch of B; the packed tables."""
    from contextflow_amd.layers import _hip
    torch.manual_seed(C * 1000 + 7)
    conv, act, cpl = L.Conv1x1((C, H, W)), L.ActNorm((C, H, W)), L.Coupling(C, kernel_size=(3, 3), padding=(1, 1))
    with torch.no_grad():
        conv.NN.add_(0.1 * torch.randn(C, C))
        act.NN_t.copy_(0.3 * torch.randn(C)); act.NN_logs.copy_(0.2 * torch.randn(C)); act.initialized.fill_(1)
    act._init_done = True
    x = torch.randn(B, C, H, W)
    cpu = (conv.NN.detach().double(), act.NN_t.detach().double(), act.NN_logs.detach().double(),
           {"0." + k: v.detach().double() for k, v in cpl.state_dict().items()})
    for m in (conv, act, cpl):
        m.to(DEV)
    f, pp = _hip.f32, _hip.p
    ws = torch.empty(_hip.lib().cf_flow_step_ws_bytes(C, H, W), device=DEV, dtype=torch.uint8)
    c1, c2, c3 = cpl.NN[0], cpl.NN[2], cpl.NN[4]
    _hip.call("cf_flow_step_prepare", pp(f(conv.NN.detach())), pp(f(act.NN_t.detach())), pp(f(act.NN_logs.detach())),
              pp(f(c1.weight.detach())), pp(f(c1.bias.detach())), pp(f(c2.weight.detach())), pp(f(c2.bias.detach())),
              pp(f(c3.weight.detach())), pp(f(c3.bias.detach())), pp(ws), C, H, W, _hip.stream())
    return x, ws, cpu


@pytest.mark.gpu
@pytest.mark.parametrize("squeeze", [False, True])
@pytest.mark.parametrize("B", [15, 16, 17, 33, 48])
def test_zero_skip_kernel_equals_the_2x4_kernel_bitwise(L, B, squeeze):
    """Variant 7 against variant 6 on the same tables: z and a pre-seeded, non-zero running log-det, bit for bit.  15: one partial
    workgroup; 16: one; 17: a full one and one sample; 33, 48: more.  At 17 also against the fp64 oracle of the step, under the
    bars of tests/test_winograd24.py: z to 1e-5 of its scale, the log-det to 1e-5 relative."""
    x, ws, (Wm, t, logs, p) = seeded_step(L, B)
    xin = (fo.squeeze_inv(x, (2, 2)) if squeeze else x).to(DEV).contiguous()
    ldj0 = torch.linspace(-3.0, 5.0, B, device=DEV)
    z6, l6 = step_variant(xin, ws, ldj0, squeeze, 6)
    z7, l7 = step_variant(xin, ws, ldj0, squeeze, 7)
    assert not torch.isnan(z7).any()
    assert torch.equal(z7, z6)
    assert torch.equal(l7, l6) and not torch.equal(l7, ldj0)
    if B == 17:
        y, l0 = fo.conv1x1_fwd(x.double(), Wm)
        y, l1 = fo.actnorm_fwd(y, t, logs)
        zref, l2 = fo.coupling_fwd(y, p, "0.", (1, 1))
        lref = l0 + l1 + l2
        scale = max(1.0, zref.abs().max().item())
        z7, l7 = step_variant(xin, ws, torch.zeros(B, device=DEV), squeeze, 7)      # (the step's own term, as that file reads it)
        ez = (z7.cpu().double() - zref).abs().max().item()
        el = ((l7.cpu().double() - lref).abs() / lref.abs().clamp_min(1.0)).max().item()
        print("B=17 squeeze=%d: z err / scale %.3g, ldj rel %.3g" % (squeeze, ez / scale, el))
        assert ez <= 1e-5 * scale
        assert el <= 1e-5


@pytest.mark.gpu
def test_log_prob_above_the_threshold_is_bitwise_what_it_is_with_the_kernel_off(L):
    """The cifar10 fixtures tiled to the first batch at which cf_flow_step_fwd takes the zero-skipping kernel, through the
    evaluation forward with the kernel on (default) and off (the hook cf_flow_step_zero_skip_enable): the same bits."""
    from tests.gpu_util import build_model, set_noise
    from contextflow_amd.layers import _hip
    q, enable = _hip.lib().cf_flow_step_zero_skip_min_batch, _hip.lib().cf_flow_step_zero_skip_enable
    q.restype, q.argtypes = ctypes.c_int, [ctypes.c_int] * 3
    enable.restype, enable.argtypes = ctypes.c_int, [ctypes.c_int]
    assert os.environ.get("CONTEXTFLOW_DIRECT_CONV") != "1"
    minb = q(C, H, W)
    assert minb > 8192, minb              # on by default, above every batch at which a test pins the 4x4 level's kernel
    name = "cifar10"
    ops, _, M, params, fx = load_e2e(name, None)
    x, u, eps = e2e_inputs(name, fx)
    rep = -(-minb // x.shape[0])
    B = x.shape[0] * rep
    model = build_model(name, params)
    # (tiled on the device: the batch is 0.8 GB of input)
    set_noise(model, u.to(DEV).repeat(rep, 1, 1, 1), [e.to(DEV).repeat(rep, *([1] * (e.dim() - 1))) for e in eps])
    xd = x.to(DEV).repeat(rep, 1, 1, 1)

    def run():
        model.step_events = []
        try:
            with torch.no_grad():
                z, logp = model(xd)
            torch.cuda.synchronize()
            launches = [(e[2], e[3], e[4]) for e in model.step_events]
        finally:
            model.step_events = None
        assert launches.count((B, C, HW)) == 4, launches      # the 4x4 level's steps went through cf_flow_step_fwd
        return z.clone(), logp.clone()

    z_on, lp_on = run()
    assert enable(0) == 1                 # it was on: the default
    try:
        assert q(C, H, W) == 0
        z_off, lp_off = run()
    finally:
        enable(1)
    assert q(C, H, W) == minb
    assert torch.equal(lp_on, lp_off) and torch.equal(z_on, z_off)
    assert torch.isfinite(lp_on).all()
