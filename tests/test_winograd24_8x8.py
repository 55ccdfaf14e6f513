"""The Winograd F(2x4, 3x3) form of the coupling nets' 3x3 on the 8x8 level (contextflow_amd/csrc/cf_step_common.h:
winograd24_phase2 at Geo<32, 8, 8, 4, 6>).  CPU: the end-to-end fixtures through the oracle with the 3x3 in the production
forms (F(2x4) on 4x4 and 8x8 images, F(2x2) on 16x16), the h1 order of the 8x8 geometry (index maps and LDS banks), the
executed multiply-add counts of the dispatch.  GPU: the step kernel at batches with a partially filled last workgroup and
column tile, and the mnist fixtures tiled to 4096 samples."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import flow_oracle as fo
from oracle.winograd import winograd3x3_reflect
from tests.helpers import load_e2e, e2e_inputs, bpd, stress_tolerance
from tests.test_winograd24 import winograd24_3x3_reflect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BPD_TOL = 1e-5
DEV = "cuda:0"
MIN_B = 2048             # smallest batch at which the 8x8 level runs the F(2x4) form


def coupling_net_production(x0, p, prefix, pad):
    """oracle.flow_oracle.coupling_net with the 3x3 in the forms the evaluation forward runs at saturating batches:
    F(2x4, 3x3) on 4x4 and 8x8 images, F(2x2, 3x3) on 16x16 images."""
    h = F.relu(F.conv2d(x0, p[prefix + "NN.0.weight"], p[prefix + "NN.0.bias"]))
    assert h.dtype == torch.float32 and tuple(pad) == (1, 1)
    conv = winograd24_3x3_reflect if tuple(h.shape[2:]) in ((4, 4), (8, 8)) else winograd3x3_reflect
    h = F.relu(conv(h, p[prefix + "NN.2.weight"], p[prefix + "NN.2.bias"]))
    return F.conv2d(h, p[prefix + "NN.4.weight"], p[prefix + "NN.4.bias"])


@pytest.mark.parametrize("tag", [None, "stress", "extreme"])
@pytest.mark.parametrize("name,n8", [("cifar10", 4), ("mnist", 2)])
def test_e2e_fixtures_with_the_2x4_form_on_the_4x4_and_8x8_levels(name, n8, tag):
    """bits/dim within the fixtures' bars of the reference's fp32 and fp64 results in every regime; the 8x8 couplings took
    the F(2x4) form."""
    ops, _, M, params, fx = load_e2e(name, tag)
    x, u, eps = e2e_inputs(name, fx)
    tol = stress_tolerance(fx, tag) if tag else BPD_TOL
    direct, calls = fo.coupling_net, []

    def counted(x0, p, prefix, pad):
        calls.append(tuple(x0.shape[2:]))
        return coupling_net_production(x0, p, prefix, pad)
    try:
        fo.coupling_net = counted
        _, logp = fo.flow_forward(ops, params, x, u, eps)
    finally:
        fo.coupling_net = direct
    assert calls.count((8, 8)) == n8, calls
    for key in ("logp", "logp_f64"):
        if key in fx:
            err = (bpd(logp, name) - bpd(torch.from_numpy(fx[key]), name)).abs().max().item()
            print("%s %s vs %s: max |d bits/dim| = %.3g (bar %.3g)" % (name, tag, key, err, tol))
            assert err < tol, key


# ---- the h1 order of the 8x8 geometry: a restatement of w24_row / w24_col / w24_pix and of the lane maps of phases 1 and 2
H = W = 8
SPW, PIX, HW = 4, 256, 64


def w24_row(s, y, kq):
    return 128 * (s >> 1) + 32 * ((y ^ (kq >> 1)) & 1) + 8 * (y >> 1) + 4 * (s & 1)


def w24_col(x, kq):
    return 64 * ((x >> 1) & 1) + 2 * (((x >> 2) ^ (x >> 1)) & 1) + ((x ^ kq) & 1)


def reflect(v, n):
    return -v if v < 0 else (2 * (n - 1) - v if v >= n else v)


def lane_tile(wave, lane):
    """(sample, tile row, tile column, first 16-row tile) of a lane of winograd24_phase2: 16 tiles of 2x4 pixels per column
    tile, two column tiles, the two waves of a column tile split the four 16-row tiles."""
    tg = (wave % 2) * 16 + (lane & 15)
    return tg // 8, (tg % 8) // 2, tg % 2, (wave // 2) * 2


def test_h1_order_every_pixel_written_once():
    """Phase 1 writes pixel (s, y, x) of row k at word w24_pix(s, y, x, k & 3) of the row: a bijection onto the 256 words
    for every k & 3, so h2 (natural order, written after a barrier) and h1 never share a half-written row."""
    for kq in range(4):
        words = sorted(w24_row(s, y, kq) + w24_col(x, kq) for s in range(SPW) for y in range(H) for x in range(W))
        assert words == list(range(PIX)), kq


def test_h1_order_patch_reads_and_banks():
    """Every patch element (a, c) of every lane is read from the pixel the reflect padding names, and one read (16 tiles x 4
    consecutive rows k) is conflict-free both ways of counting: as the hardware serves a ds_read_b32 (two groups of 32
    lanes, bank = word address mod 32) and as 64 lanes on 64 banks; lanes with the same word aside (a broadcast)."""
    ident = torch.arange(SPW * HW, dtype=torch.float32).reshape(SPW, 1, H, W)             # pixel ids
    patches = F.pad(ident, (1, 1, 1, 1), mode="reflect").unfold(2, 4, 2).unfold(3, 6, 4)   # (s, 1, ty, tx, 4, 6)
    planes = []                                      # plane[kq][word] = pixel id, as phase 1 leaves it
    for kq in range(4):
        pl = [None] * PIX
        for s in range(SPW):
            for y in range(H):
                for x in range(W):
                    pl[w24_row(s, y, kq) + w24_col(x, kq)] = s * HW + y * W + x
        planes.append(pl)
    covered = set()
    for wave in range(4):
        for a in range(4):
            for c in range(6):
                addr = {}
                for lane in range(64):
                    s, ty, tx, rt0 = lane_tile(wave, lane)
                    kq = lane >> 4                   # rows 16 kk + 8 e2 + 4 j + (lane >> 4): k & 3 = lane >> 4
                    word = w24_row(s, reflect(2 * ty - 1 + a, H), kq) + w24_col(reflect(4 * tx - 1 + c, W), kq)
                    assert planes[kq][word] == int(patches[s, 0, ty, tx, a, c]), (wave, lane, a, c)
                    addr[lane] = kq * PIX + word
                    covered.add((s, ty, tx, rt0))
                for group, nb in ((range(0, 32), 32), (range(32, 64), 32), (range(64), 64)):
                    banks = {}
                    for lane in group:
                        assert banks.setdefault(addr[lane] % nb, addr[lane]) == addr[lane], ("bank conflict", wave, a, c, lane, nb)
    # every output tile of the four samples has an owner for each half of the 16-row tiles
    assert covered == {(s, ty, tx, rt0) for s in range(SPW) for ty in range(4) for tx in range(2) for rt0 in (0, 2)}


# ---- the dispatch's executed multiply-adds ---------------------------------------------------------------------------
MACS_SCRIPT = """
import sys
sys.path.insert(0, %r)
from contextflow_amd.layers import _hip
L = _hip.lib()
print(" ".join(str(L.cf_flow_step_macs(b, 32, 8, 8, p)) for b in (1024, 2047, 2048, 4101, 1 << 21) for p in (0, 1, 2, 3)))
"""


def macs_table(env):
    from contextflow_amd import build
    build.build()
    e = {k: v for k, v in os.environ.items() if not k.startswith("CONTEXTFLOW_")}
    r = subprocess.run([sys.executable, "-c", MACS_SCRIPT % ROOT], env=dict(e, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    v = [int(t) for t in r.stdout.split()]
    return {(b, p): v[i * 4 + p] for i, b in enumerate((1024, 2047, 2048, 4101, 1 << 21)) for p in range(4)}


def test_executed_macs_of_the_8x8_level():
    """20 C^2 HW below 2048 samples, 16 C^2 HW from there on in the evaluation forward (pass 0); the taped forward, the
    backward and the inverse (passes 1-3) are what they were."""
    unit = 32 * 32 * 64
    on = macs_table({})
    for b in (1024, 2047, 2048, 4101, 1 << 21):
        assert on[b, 0] == (16 if b >= MIN_B else 20) * unit, b
        assert (on[b, 1], on[b, 2], on[b, 3]) == (20 * unit, 40 * unit, 20 * unit), b


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


def step_variant(x, ws, C, Hh, Ww, squeeze, variant):
    """cf_flow_step_fwd_debug without dumps: the kernel variant of the dispatch table (4 = F(2x2), 6 = F(2x4))."""
    from contextflow_amd.layers import _hip
    fn = _hip.lib().cf_flow_step_fwd_debug
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    B = x.shape[0]
    z = torch.full((B, C, Hh, Ww), float("nan"), device=x.device)
    ldj = torch.zeros(B, device=x.device)
    _hip.check(fn(_hip.p(x), _hip.p(z), _hip.p(ldj), _hip.p(ws), B, C, Hh, Ww, C * Hh * Ww, int(squeeze), None, variant << 16,
                  _hip.stream()), "cf_flow_step_fwd_debug")
    torch.cuda.synchronize()
    return z, ldj


@pytest.mark.gpu
@pytest.mark.parametrize("squeeze", [False, True])
@pytest.mark.parametrize("B", [4099, 4101])
def test_the_8x8_step_kernel_with_partial_workgroup_and_column_tile(L, B, squeeze):
    """One fused step of the 8x8 level through the production entry point at 4099 / 4101 samples (the last workgroup holds
    3 / 1 of its 4 samples: a full and a half-empty column tile / one half-filled column tile), against the fp64 oracle of
    the step - z to 1e-5 of its scale, the log-det to 1e-5 relative - and against the F(2x2) kernel: both sit within the
    oracle bar, so they differ by at most twice that."""
    from contextflow_amd.layers import _hip
    C, Hh, Ww = 32, 8, 8
    assert _hip.lib().cf_flow_step_macs(B, C, Hh, Ww, 0) == 16 * C * C * Hh * Ww
    torch.manual_seed(B)
    conv, act, cpl = L.Conv1x1((C, Hh, Ww)), L.ActNorm((C, Hh, Ww)), L.Coupling(C, kernel_size=(3, 3), padding=(1, 1))
    with torch.no_grad():
        conv.NN.add_(0.1 * torch.randn(C, C))
        act.NN_t.copy_(0.3 * torch.randn(C)); act.NN_logs.copy_(0.2 * torch.randn(C)); act.initialized.fill_(1)
    act._init_done = True
    x = torch.randn(B, C, Hh, Ww)
    p = {"0." + k: v.detach().double() for k, v in cpl.state_dict().items()}
    y, l0 = fo.conv1x1_fwd(x.double(), conv.NN.detach().double())
    y, l1 = fo.actnorm_fwd(y, act.NN_t.detach().double(), act.NN_logs.detach().double())
    zref, l2 = fo.coupling_fwd(y, p, "0.", (1, 1))
    lref = l0 + l1 + l2
    for m in (conv, act, cpl):
        m.to(DEV)
    xin = (fo.squeeze_inv(x, (2, 2)) if squeeze else x).to(DEV).contiguous()
    f, pp = _hip.f32, _hip.p
    ws = torch.empty(_hip.lib().cf_flow_step_ws_bytes(C, Hh, Ww), device=DEV, dtype=torch.uint8)
    c1, c2, c3 = cpl.NN[0], cpl.NN[2], cpl.NN[4]
    _hip.call("cf_flow_step_prepare", pp(f(conv.NN.detach())), pp(f(act.NN_t.detach())), pp(f(act.NN_logs.detach())),
              pp(f(c1.weight.detach())), pp(f(c1.bias.detach())), pp(f(c2.weight.detach())), pp(f(c2.bias.detach())),
              pp(f(c3.weight.detach())), pp(f(c3.bias.detach())), pp(ws), C, Hh, Ww, _hip.stream())
    z_prod = torch.full((B, C, Hh, Ww), float("nan"), device=DEV)
    ldj_prod = torch.zeros(B, device=DEV)
    _hip.call("cf_flow_step_fwd", pp(xin), pp(z_prod), pp(ldj_prod), pp(ws), B, C, Hh, Ww, C * Hh * Ww, int(squeeze), _hip.stream())
    torch.cuda.synchronize()
    z24, ldj24 = step_variant(xin, ws, C, Hh, Ww, squeeze, 6)
    z22, ldj22 = step_variant(xin, ws, C, Hh, Ww, squeeze, 4)
    # the production entry point IS the F(2x4) kernel at this batch (same launch, same arithmetic: bitwise)
    assert torch.equal(z_prod, z24) and torch.equal(ldj_prod, ldj24)
    assert not torch.equal(z24, z22)                 # ... and not the F(2x2) one
    scale = max(1.0, zref.abs().max().item())
    rel = lambda l: ((l.cpu().double() - lref).abs() / lref.abs().clamp_min(1.0)).max().item()
    ez24, ez22 = (z24.cpu().double() - zref).abs().max().item(), (z22.cpu().double() - zref).abs().max().item()
    ezz = (z24 - z22).abs().max().item()
    print("B=%d squeeze=%d: z err / scale  F(2x4) %.3g  F(2x2) %.3g  between %.3g;  ldj rel  F(2x4) %.3g  F(2x2) %.3g"
          % (B, squeeze, ez24 / scale, ez22 / scale, ezz / scale, rel(ldj24), rel(ldj22)))
    assert ez24 <= 1e-5 * scale and rel(ldj24) <= 1e-5
    assert ezz <= 2e-5 * scale
    assert ((ldj24 - ldj22).abs().cpu().double() / lref.abs().clamp_min(1.0)).max().item() <= 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("tag", [None, "stress", "extreme"])
def test_mnist_fixtures_tiled_to_4096_samples(L, tag):
    """The mnist fixtures' samples and captured noise repeated to 4096 rows through the evaluation forward: the 8x8 level's
    two steps run the F(2x4) kernel and every row reproduces the reference's log-density within the end-to-end bars."""
    from tests.gpu_util import build_model, set_noise
    from contextflow_amd.layers import _hip
    name = "mnist"
    ops, _, M, params, fx = load_e2e(name, tag)
    x, u, eps = e2e_inputs(name, fx)
    rep = 4096 // x.shape[0]
    B = x.shape[0] * rep
    assert B >= MIN_B
    tol = stress_tolerance(fx, tag) if tag else BPD_TOL
    model = build_model(name, params)
    set_noise(model, None if u is None else u.repeat(rep, 1, 1, 1), [e.repeat(rep, *([1] * (e.dim() - 1))) for e in eps])
    model.step_events = []            # (start, end, batch, C, H*W) per cf_flow_step_fwd launch
    try:
        with torch.no_grad():
            z, logp = model(x.repeat(rep, 1, 1, 1).to(DEV))
        torch.cuda.synchronize()
        launches = [(e[2], e[3], e[4]) for e in model.step_events]
    finally:
        model.step_events = None
    assert launches.count((B, 32, 64)) == 2, launches
    assert _hip.lib().cf_flow_step_macs(B, 32, 8, 8, 0) == 16 * 32 * 32 * 64
    lp = logp.cpu()
    for key in ("logp", "logp_f64"):
        if key in fx:
            ref = torch.from_numpy(fx[key]).repeat(rep, 1)
            err = (bpd(lp, name) - bpd(ref, name)).abs().max().item()
            print("mnist %s vs %s: max |d bits/dim| = %.3g (bar %.3g)" % (tag, key, err, tol))
            assert err < tol, key
    zr = torch.from_numpy(fx["z"]).repeat(rep, *([1] * (fx["z"].ndim - 1)))
    assert (z.cpu() - zr).abs().max().item() <= 2e-4 * max(1.0, zr.abs().max().item())
