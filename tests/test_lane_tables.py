"""Per-lane address tables of the flow-step kernels (csrc/cf_step_common.h: LaneTab).

Host: every entry of the compiled-in tables (debug entry cf_lane_table_debug) equals the value the documented formulas give for every
(wave, lane) of each geometry, rebuilt here in Python.

GPU (run with -m gpu): sha256 of z and of the running log-det on seeded inputs, for every kernel form that shares the tabulated
bodies - the single-step kernel (debug entry, forced variant) and the level kernel with 1 and 4 steps, plain and squeeze-folded, at
batches with full and ragged last workgroups.  The digests in tests/golden/lane_tables_sha256.json were recorded on an MI355X from the
library as it was BEFORE the tables existed (commit d8460e4): the tables may change how an address is obtained, never a bit of the
result.  Inputs come from seeded CPU generators and every sum in these kernels has a fixed order, so the digests hold from run to run."""
import ctypes
import hashlib
import json
import os

import pytest
import torch

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lane_tables_sha256.json")

# (C, H, W), batches, debug variants of the single-step form (kDebugKernel in csrc/cf_step.hip: 4 = Winograd F(2x2) in
# k_flow_step_small, 5 = F(2x2) row-split at 128 pixels per workgroup, 6 = F(2x4)).  16x16: one sample per workgroup; 8x8: 4 per
# workgroup, ragged (3, 5, 9) and full (4); 4x4: 8 per workgroup, ragged (7, 9, 17) and full (8).  The 4x4 level runs the F(2x4)
# geometry (variant 6); variant 5 shares winograd_phase2 with the 16x16 level and is hashed as well.
GEOMETRIES = [((16, 16, 16), (1, 3), (4,)), ((32, 8, 8), (3, 4, 5, 9), (6,)), ((64, 4, 4), (7, 8, 9, 17), (5, 6))]
CASES = [(shape, B, squeeze, form) for shape, Bs, variants in GEOMETRIES for B in Bs for squeeze in (False, True)
         for form in ["level1", "level4"] + ["single%d" % v for v in variants]]


def case_key(shape, B, squeeze, form):
    return "%dx%dx%d/B%d/%s/%s" % (shape + (B, "squeeze" if squeeze else "plain", form))


# ---- host: the tables against the documented formulas ----------------------------------------------------------------------------
def reflect(v, n):
    return -v if v < 0 else (2 * (n - 1) - v if v >= n else v)


def w24_row(s, y, kq):          # cf_step_common.h: word of pixel (s, y, x) inside row k of the 8x8 h1 plane = row part + column part
    return 128 * (s >> 1) + 32 * ((y ^ (kq >> 1)) & 1) + 8 * (y >> 1) + 4 * (s & 1)


def w24_col(x, kq):
    return 64 * ((x >> 1) & 1) + 2 * (((x >> 2) ^ (x >> 1)) & 1) + ((x ^ kq) & 1)


def entry_8x8(wave, lane):
    """Geo<32, 8, 8, 4, 6>: 4 samples = 256 pixels per workgroup, two column tiles of 16 output tiles (2x4 pixels); wave w takes
    column tile w & 1.  Lane: tile l15 of the column tile, k row lg of a group of four."""
    C, H, W, SPW = 32, 8, 8, 4
    HW, PIX, HALF, PTW = H * W, SPW * H * W, C // 2, 2
    l15, lg, li = lane & 15, lane >> 4, lane & 31
    tg = (wave % 2) * 16 + l15
    smp, ty, tx = tg // 8, (tg % 8) // 2, tg % 2
    row = [4 * w24_row(smp, reflect(2 * ty - 1 + a, H), lg) for a in range(4)]
    col = [4 * (HALF * PIX + lg * PIX + w24_col(reflect(4 * tx - 1 + c, W), lg)) for c in range(6)]
    dst = 4 * lg * PIX + smp * HW + 2 * ty * W + 4 * tx
    pw = []
    for q in range(PTW):
        pix = (wave * PTW + q) * 32 + li
        s, y, x = pix // HW, (pix % HW) // W, pix % W
        pw += [w24_row(s, y, kq) + w24_col(x, kq) for kq in range(4)]
    return row + col + [dst, 0] + pw


def entry_16x16(wave, lane):
    """Geo<16, 16, 16, 1, 3>: one sample = 256 pixels per workgroup, F(2x2): wave w owns the 16 output tiles (2x2 pixels) w 16 .. of
    the 8 x 8 tiles of the image.  h1 order: rows and columns split by parity, odd k rows in the other column-parity block."""
    C, H, W = 16, 16, 16
    HW = PIX = H * W
    HALF, PTW = C // 2, 2
    l15, lg, li = lane & 15, lane >> 4, lane & 31
    wino = lambda y, x: (y & 1) * (HW // 2) + (y >> 1) * W + (x & 1) * (W // 2) + (x >> 1)
    tg = wave * 16 + l15
    ty, tx = tg // (W // 2), tg % (W // 2)
    row, col = [], []
    for a in range(4):
        yy, xx = reflect(2 * ty - 1 + a, H), reflect(2 * tx - 1 + a, W)
        row.append(4 * (HALF * PIX + lg * PIX + wino(yy, 0)))
        col.append(4 * (((xx ^ lg) & 1) * (W // 2) + (xx >> 1)))
    pw = []
    for q in range(PTW):
        pix = (wave * PTW + q) * 32 + li
        pw.append(wino(pix // W, pix % W))
    dst = 4 * lg * PIX + 2 * ty * W + 2 * tx
    return row + col + pw + [dst, 0]


# shape -> the entry of (wave, lane); a shape that is not listed derives its addresses in the kernel and has no table (4x4: the table
# form measured slower than deriving, profiles/lane_tables.md; C = 8: its phase 1 is not the shared one)
TABLES = {(16, 16, 16): entry_16x16, (32, 8, 8): entry_8x8}


@pytest.mark.parametrize("shape", [(8, 16, 16), (16, 16, 16), (32, 8, 8), (64, 4, 4)])
def test_table_entries_equal_the_derived_values(shape):
    from contextflow_amd import build
    build.build()
    from contextflow_amd.layers import _hip
    fn = _hip.lib().cf_lane_table_debug
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_int]
    n = fn(*shape, None, 0)
    if shape not in TABLES:
        assert n == 0
        return
    want = [TABLES[shape](t >> 6, t & 63) for t in range(256)]
    assert n == len(want[0]) and n % 4 == 0          # whole 16-byte words
    buf = (ctypes.c_int * (256 * n))()
    assert fn(*shape, buf, 256 * n) == n
    got = list(buf)
    for t in range(256):
        assert got[t * n:(t + 1) * n] == want[t], (shape, t >> 6, t & 63)
    # every phase-1 word stays inside its row, every phase-2 read inside the h1 planes (8x8: rows HALF .. HALF + 4 of the k group)
    if shape == (32, 8, 8):
        for e in want:
            assert all(0 <= w < 256 for w in e[12:20])
            lo, hi = 4 * 16 * 256, 4 * (16 + 4) * 256
            assert all(lo <= r + c < hi for r in e[0:4] for c in e[4:10])
    if shape == (16, 16, 16):
        for e in want:
            assert all(0 <= w < 256 and 0 <= (w ^ 8) < 256 for w in e[8:10])
            lo, hi = 4 * 8 * 256, 4 * (8 + 4) * 256
            assert all(lo <= r + c < hi for r in e[0:4] for c in e[4:8])


_tables = {}


def step_tables(shape):
    """Four packed step tables of `shape` from a seeded CPU generator (made once per shape, never written again)."""
    from contextflow_amd.layers import _hip
    if shape in _tables:
        return _tables[shape]
    C, H, W = shape
    HALF, HID = C // 2, 2 * C
    f, pp = _hip.f32, _hip.p
    out = []
    for i in range(4):
        g = torch.Generator().manual_seed(5000 * C + i)
        rn = lambda *s: torch.randn(*s, generator=g)
        host = [torch.eye(C) + 0.1 * rn(C, C), 0.3 * rn(C), 0.2 * rn(C),
                rn(HID, HALF, 1, 1) / HALF ** 0.5, 0.05 * rn(HID), rn(HID, HID, 3, 3) / (9 * HID) ** 0.5, 0.05 * rn(HID),
                0.5 * rn(C, HID, 1, 1) / HID ** 0.5, 0.05 * rn(C)]
        dev = [t.to(DEV) for t in host]
        ws = torch.empty(_hip.lib().cf_flow_step_ws_bytes(C, H, W), device=DEV, dtype=torch.uint8)
        _hip.call("cf_flow_step_prepare", *[pp(f(t)) for t in dev], pp(ws), C, H, W, _hip.stream())
        out.append(ws)
    torch.cuda.synchronize()
    _tables[shape] = out
    return out


def run_case(shape, B, squeeze, form):
    """(z, ldj) of one case on seeded inputs."""
    from contextflow_amd.layers import _hip
    lib = _hip.lib()
    C, H, W = shape
    N = C * H * W
    tabs = step_tables(shape)
    g = torch.Generator().manual_seed(977 * C + B)
    xh = torch.randn(B, N, generator=g)
    ldj = (torch.randn(B, generator=g) + 3.0).to(DEV)
    x = xh.to(DEV).view(B, C // 4, 2 * H, 2 * W) if squeeze else xh.to(DEV).view(B, C, H, W)
    z = torch.full((B, C, H, W), float("nan"), device=DEV)
    if form.startswith("level"):
        n = int(form[5:])
        rc = lib.cf_flow_step_fwd_level(_hip.p(x), _hip.p(z), _hip.p(ldj), _hip.ptr_array(tabs[:n]), n, B, C, H, W, N, int(squeeze), 1,
                                        _hip.stream())
        _hip.check(rc, "cf_flow_step_fwd_level")
    else:
        fn = lib.cf_flow_step_fwd_debug
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        _hip.check(fn(_hip.p(x), _hip.p(z), _hip.p(ldj), _hip.p(tabs[0]), B, C, H, W, N, int(squeeze), None, int(form[6:]) << 16,
                      _hip.stream()), "cf_flow_step_fwd_debug")
    torch.cuda.synchronize()
    return z, ldj


def digest(z, ldj):
    h = hashlib.sha256()
    for t in (z, ldj):
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def all_digests():
    """{case key: sha256}: what tests/golden/lane_tables_sha256.json holds (recorded with this function on the parent commit)."""
    return {case_key(*c): digest(*run_case(*c)) for c in CASES}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,B,squeeze,form", CASES, ids=[case_key(*c) for c in CASES])
def test_bits_unchanged(golden, shape, B, squeeze, form):
    z, ldj = run_case(shape, B, squeeze, form)
    assert torch.isfinite(z).all() and torch.isfinite(ldj).all()
    got = digest(z, ldj)
    print("LANE_TABLES_SHA %s %s" % (case_key(shape, B, squeeze, form), got))
    assert golden.get(case_key(shape, B, squeeze, form)) == got
