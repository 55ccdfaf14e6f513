"""CPU tests (no GPU): the C-ABI library loads and exports every declared symbol, the host-side
mirror of the reference API has the reference's state_dict layout, the product refuses to run on
the CPU (no silent fallback), and the multi-rank NLL reduction is correct (gloo, world size 2)."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from contextflow_amd import build
    return build.build()


def header_symbols():
    src = open(os.path.join(ROOT, "include", "contextflow_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(cf_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(built):
    import ctypes
    from contextflow_amd.layers import _hip
    syms = header_symbols()
    assert len(syms) >= 30
    lib = ctypes.CDLL(built)
    for s in syms:
        assert hasattr(lib, s), "header declares %s but the library does not export it" % s
    assert sorted(_hip.SIGNATURES) == syms, set(_hip.SIGNATURES) ^ set(syms)
    assert _hip.lib().cf_abi_version() == _hip.ABI_VERSION == 16
    # pure host-side queries work without a GPU
    assert _hip.lib().cf_flow_step_supported(64, 4, 4, 3, 3) == 1
    assert _hip.lib().cf_flow_step_supported(26, 8, 1, 3, 1) == 0
    assert _hip.lib().cf_flow_step_ws_bytes(16, 16, 16) > 4 * 10064
    assert _hip.lib().cf_actnorm_stats_ws_bytes(16) == 16 * 65 * 2 * 8


def test_host_side_size_queries_of_round_3(built):
    """Host-only entry points (no GPU call): executed multiply-adds of the step kernels as dispatched, the plane / partial
    buffer sizes of the transformer step backward (the Python side slices the plane buffer by the layout of the header),
    the grouped weight gradient's workspace."""
    import ctypes
    from contextflow_amd.layers import _hip
    L = _hip.lib()
    direct = lambda C, H: 40 * C * C * H * H
    # evaluation forward: Winograd at 16x16 always, at 8x8 / 4x4 from 1024 / 2048 samples; backward: direct; weight gradients: Winograd
    assert L.cf_flow_step_macs(256, 16, 16, 16, 0) == direct(16, 16) // 2
    assert L.cf_flow_step_macs(256, 32, 8, 8, 0) == direct(32, 8) and L.cf_flow_step_macs(1024, 32, 8, 8, 0) == direct(32, 8) // 2
    assert L.cf_flow_step_macs(2047, 64, 4, 4, 1) == direct(64, 4) and L.cf_flow_step_macs(2048, 64, 4, 4, 1) == direct(64, 4) // 2
    assert L.cf_flow_step_macs(256, 8, 16, 16, 0) == direct(8, 16) // 2 and L.cf_flow_step_macs(256, 8, 16, 16, 1) == direct(8, 16)
    assert L.cf_flow_step_macs(4096, 16, 16, 16, 2) == direct(16, 16)
    assert L.cf_step_wgrads_macs(4096, 32, 8, 8) == direct(32, 8) // 2
    assert L.cf_flow_step_macs(4096, 26, 8, 1, 0) == 0                     # not a conv-step shape
    # transformer step backward: B = 10 -> Bp = 12: planes [x^T, g_y (8 Bp, 26)] [u0 (4 Bp, 26), g_e (4 Bp, 52)] + depth x 4 Bp x 568
    B, C, depth = 10, 26, 6
    Bp = 12
    assert L.cf_vit_step_bwd_plane_floats(B, C, depth) == 2 * 8 * Bp * 26 + 4 * Bp * (26 + 52) + depth * 4 * Bp * 568
    assert L.cf_vit_step_bwd_ln_floats(B, C, depth) == 3 * (64 + 128 + depth * 256 + 128)
    assert L.cf_vit_step_bwd_ws_bytes(C, depth) > 4 * depth * (192 * 52 + 52 * 64 + 2 * 52 * 52)
    assert L.cf_vit_step_supported(26, 8, 1, 2, 1, 52, 64, 1, 6) == 1 and L.cf_vit_step_supported(38, 144, 1, 2, 1, 76, 64, 1, 6) == 0
    assert L.cf_vit_step_supported(26, 8, 1, 2, 1, 52, 64, 1, 1) == 1 and L.cf_vit_step_supported(26, 8, 1, 2, 1, 52, 64, 1, 7) == 0
    arr = lambda v: (ctypes.c_int * len(v))(*v)
    # grouped weight gradients: partials [N][K] | [N] per row range; about 4096 waves per group, >= 64 rows per range
    one = L.cf_linear_wgrad_group_ws_bytes(arr([4096]), arr([52]), arr([192]), 1)
    assert one == 64 * (192 * 52 + 192) * 4                                # 4096 rows in ranges of 64
    many = L.cf_linear_wgrad_group_ws_bytes(arr([131072] * 26), arr([52] * 26), arr([192] * 26), 26)
    assert many == 26 * 79 * (192 * 52 + 192) * 4                          # 52 tile groups -> 79 ranges (of 1664 rows) per member
    assert L.cf_linear_wgrad_group_ws_bytes(arr([1]), arr([1]), arr([1]), 0) == -1


def test_vit_step_family_sizes_and_symbols(built):
    """The transformer flow step has one entry-point family with a `form` argument (ABI 16).  Its host-only queries give what
    the per-form functions of ABI 15 gave (literals read from that library), the flat parameter count is the one
    TransCoupling._flat_params_build produces, and the per-form / `_taped` / single-step names are gone from the header and
    from the ctypes table."""
    import contextflow_amd.layers as CL
    from contextflow_amd.layers import _hip
    from tests.helpers import unit
    L = _hip.lib()
    WAVE, RS = CL.TransCoupling.STEP_FORMS["wave"], CL.TransCoupling.STEP_FORMS["rs"]
    assert (WAVE, RS) == (0, 1)
    assert L.cf_vit_step_ws_bytes(26, 6, WAVE) == 507344           # cf_vit_step_ws_bytes(26, 6) of ABI 15
    assert L.cf_vit_step_ws_bytes(26, 6, RS) == 944208             # cf_vit_step_rs_ws_bytes(26, 6)
    assert L.cf_vit_step_ws_bytes(26, 6, 2) == 0 and L.cf_vit_step_ws_bytes(24, 6, RS) == 0
    assert L.cf_vit_step_bwd_ws_bytes(26, 6) == 608512
    assert L.cf_vit_step_tape_floats(37, 26, 6) == 93184 == 7 * 52 * L.cf_vit_step_tape_tokens(37)
    assert L.cf_vit_step_chain_max_steps() == 8                    # cf_vit_step_rs_chain_max_steps()
    t, sd = unit("trans_ts")
    m = CL.TransCoupling(tuple(int(v) for v in t["in_sz"]), tuple(int(v) for v in t["p"]))
    m.load_state_dict(sd)
    assert m._flat_params_build().numel() == L.cf_vit_flat_params(26, 52, 6) == 115856
    gone = ["cf_vit_step_prepare", "cf_vit_step_fwd_taped", "cf_vit_step_bwd_prepare", "cf_vit_step_bwd_taped", "cf_vit_step_rs_supported",
            "cf_vit_step_rs_ws_bytes", "cf_vit_step_rs_prepare", "cf_vit_step_rs_prepare_batch", "cf_vit_step_rs_fwd",
            "cf_vit_step_rs_fwd_taped", "cf_vit_step_rs_fwd_chain", "cf_vit_step_rs_chain_max_steps"]
    syms = header_symbols()
    for name in gone:
        assert name not in syms and name not in _hip.SIGNATURES, name
    assert sum(s.startswith("cf_vit_step") for s in syms) == 14


def test_csrc_units_include_headers_only():
    """A kernel family that more than one translation unit instantiates is a header: no file under csrc/ includes a .hip or is
    cut down by a ..._KERNELS_ONLY macro, and every header's first line of code is `#pragma once` (a fragment that is meant to
    be included more than once is no .h).  cf_step.hip holds launch lists and entry points only: its kernels are in headers."""
    csrc = os.path.join(ROOT, "contextflow_amd", "csrc")
    names = sorted(os.listdir(csrc))
    assert sum(n.endswith(".hip") for n in names) >= 23 and sum(n.endswith(".h") for n in names) >= 12
    for n in names:
        text = open(os.path.join(csrc, n)).read()
        assert not re.search(r'#\s*include\s*["<][^">]*\.hip[">]', text), n
        assert "KERNELS_ONLY" not in text, n
        if n.endswith(".h"):
            code = [l.strip() for l in text.split("\n") if l.strip() and not l.strip().startswith("//")]
            assert code[0] == "#pragma once", n
    assert "__global__" not in open(os.path.join(csrc, "cf_step.hip")).read()


def test_csrc_headers_stand_alone():
    """Every header under csrc/ includes what it uses: it passes the compiler's syntax check as a translation unit of its own
    (host and device pass; nothing is instantiated, so nothing is generated)."""
    import concurrent.futures
    from contextflow_amd import build
    csrc = os.path.join(ROOT, "contextflow_amd", "csrc")
    headers = sorted(n for n in os.listdir(csrc) if n.endswith(".h"))
    assert len(headers) >= 12

    def check(n):
        cmd = ["hipcc", "--offload-arch=" + build.ARCH, "-std=c++17", "-x", "hip", "-fsyntax-only", "-Wno-pragma-once-outside-header",
               os.path.join(csrc, n)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        return n, r.returncode, r.stderr[-2000:]

    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        for n, rc, err in ex.map(check, headers):
            assert rc == 0, "%s does not compile on its own:\n%s" % (n, err)


# ---- the step dispatch as the flop accounting sees it -----------------------------------------------------------------
# (first B, multiply-adds in units of C^2 HW) of cf_flow_step_macs for B in 0..8192, per shape and pass 0..3, and the largest
# chained batch.  Recorded from the library as it was BEFORE the dispatch became one function (commit 76e3db3), per switch
# setting: the refactor must not move a breakpoint.  A setting lists only what differs from the default.
SHAPES = ((8, 16, 16), (16, 16, 16), (32, 8, 8), (64, 4, 4))
D40, W20 = [(0, 40)], [(0, 20)]
DISPATCH_DEFAULT = {
    (8, 16, 16): ([W20, D40, D40, W20], 1024),
    (16, 16, 16): ([W20, W20, D40, W20], 1024),
    (32, 8, 8): ([[(0, 40), (1024, 20), (2048, 16)], [(0, 40), (1024, 20)], D40, W20], 512),
    (64, 4, 4): ([[(0, 40), (2048, 16)], [(0, 40), (2048, 20)], D40, W20], 1024),
}
DISPATCH_SETTINGS = {
    "": {},
    "CONTEXTFLOW_DIRECT_CONV=1": {(8, 16, 16): ([D40] * 4, 0), (16, 16, 16): ([D40] * 4, 0),
                                  (32, 8, 8): ([D40] * 4, 512), (64, 4, 4): ([D40] * 4, 1024)},
}
DISPATCH_SCRIPT = """
import hashlib, sys
sys.path.insert(0, %r)
from contextflow_amd.layers import _hip
L = _hip.lib()
h = hashlib.sha256()
for C, H, W in %r:
    for p in range(4):
        bp = []
        for B in range(8193):
            m = L.cf_flow_step_macs(B, C, H, W, p)
            h.update(str(m).encode())
            assert m %% (C * C * H * W) == 0, (B, C, p, m)
            if not bp or bp[-1][1] != m // (C * C * H * W):
                bp.append((B, m // (C * C * H * W)))
        print(repr(bp))
    print(L.cf_flow_step_chain_max_batch(C, H, W))
print(h.hexdigest())
"""


@pytest.mark.parametrize("setting", list(DISPATCH_SETTINGS))
def test_step_dispatch_breakpoints(built, setting):
    """Every breakpoint of cf_flow_step_macs over B = 0..8192 and cf_flow_step_chain_max_batch, exactly, for the default
    environment and each dispatch switch (a child process each: the switches are read once per process)."""
    import ast
    env = {k: v for k, v in os.environ.items() if not k.startswith("CONTEXTFLOW_")}
    if setting:
        env.update([setting.split("=")])
    r = subprocess.run([sys.executable, "-c", DISPATCH_SCRIPT % (ROOT, SHAPES)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    want = {**DISPATCH_DEFAULT, **DISPATCH_SETTINGS[setting]}
    for i, shape in enumerate(SHAPES):
        got = [ast.literal_eval(s) for s in lines[5 * i:5 * i + 4]]
        assert (got, int(lines[5 * i + 4])) == want[shape], (setting, shape, got, lines[5 * i + 4])
    if setting == "":     # all 131 088 values, shape / pass / B ascending
        assert lines[20] == "7c2a86c3ec00086a32d855de78c909fd1fc4e762fe67234ccf36ecf20a48c0cf"


# Every environment variable the product reads.  A switch is part of the product's surface: one that selects nothing any more goes,
# and a new one is a decision, made here.  (dist.py also WRITES MASTER_ADDR / MASTER_PORT defaults for torch.distributed.)
ENVIRONMENT = {"CONTEXTFLOW_DIRECT_CONV", "CONTEXTFLOW_HIP_LIB", "CF_DIST_SINGLE_RANK", "RANK", "LOCAL_RANK", "WORLD_SIZE"}
# cf_flow_step_ws_bytes per shape with the tables of the removed 16-bit-piece kernels (25 (HID / 16) (HID / 32) 768 floats, HID = 2 C)
STEP_WS_BYTES_ABI14 = {(8, 16, 16): 51856, (16, 16, 16): 266896, (32, 8, 8): 1434384, (64, 4, 4): 6392848}


def test_environment_switches_of_the_product(built):
    import glob
    from contextflow_amd.layers import _hip
    pkg = os.path.join(ROOT, "contextflow_amd")
    names = set()
    for path in glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True):
        src = open(path).read()
        reads = re.findall(r"""\benviron\s*(?:\.get\s*\(|\[)\s*(["']\w+["'])?|\bgetenv\s*\(\s*(["']\w+["'])?""", src)
        assert all(a or b for a, b in reads), "%s reads an environment variable whose name is not a literal" % path
        names |= {(a or b)[1:-1] for a, b in reads}
    for path in glob.glob(os.path.join(pkg, "csrc", "*")):
        if os.path.isfile(path):
            names |= set(re.findall(r"""getenv\(\s*"(\w+)"\s*\)""", open(path).read()))
    assert names == ENVIRONMENT, names ^ ENVIRONMENT
    L = _hip.lib()
    for (C, H, W), ws0 in STEP_WS_BYTES_ABI14.items():
        hid = 2 * C
        assert L.cf_flow_step_ws_bytes(C, H, W) == ws0 - 25 * (hid // 16) * (hid // 32) * 768 * 4, (C, H, W)
    assert [25 * (2 * C // 16) * (2 * C // 32) * 768 * 4 for C in (8, 16, 32, 64)] == [0, 153600, 614400, 2457600]


# ---- the weight-gradient launch plan as the size queries and the flop accounting see it ----------------------------------------
# Recorded from the library as it was BEFORE cf_wgrad.hip got its one wg_plan (commit 46e84f8).  (H, MR, NR, taps): the shapes of
# tools/wgrad_bench.py, the mnist level, ragged ones.
WGRAD_WS_SHAPES = [(16, 32, 32, 9), (8, 64, 64, 9), (4, 128, 128, 9), (16, 16, 32, 1), (16, 32, 8, 1), (16, 16, 16, 1),
                   (8, 32, 64, 1), (8, 64, 16, 1), (8, 32, 32, 1), (4, 64, 128, 1), (4, 128, 32, 1), (4, 64, 64, 1),
                   (16, 8, 16, 1), (16, 16, 4, 1), (16, 8, 8, 1), (16, 16, 16, 9),
                   (4, 24, 40, 1), (4, 72, 100, 9), (16, 128, 128, 9)]
WGRAD_WS_SHA = "255337f9dfc253e38616005e0da80ea26bdfbc4508e8990b66266213533a5a1d"        # 19 shapes x B = 0..8192, ascending
WGRAD_STEP_WS_SHA = "3b8d2fe8ab4f4dd0cea04a09f783784756a771756d78e5bbd7d2d85071b86b02"   # SHAPES x B = 0..8192
# where the slope of the partial count over B changes: the count's change points as arithmetic runs (first B, spacing, step,
# how many).  Staged 3x3 at 4x4: a split per 4 chunks of 4 samples up to 512 / 4 row tiles; the skinny 1x1: one partial per four
# waves of qper units, qper growing by one every 1024 / 2048 samples (each time the count falls back)
WGRAD_WS_RUNS = {
    (4, 128, 128, 9): [(29, 16, 1, 127)],
    (8, 32, 64, 1): [(3, 2, 1, 511), (1025, 0, -255, 1), (1029, 4, 1, 255)],
    (4, 24, 40, 1): [(5, 4, 1, 511), (2049, 0, -255, 1), (2057, 8, 1, 255), (4097, 0, -170, 1), (4105, 12, 1, 170),
                     (6145, 0, -127, 1), (6161, 16, 1, 127)],
}


def _runs(S):
    out = []
    for B in range(1, len(S)):
        d = S[B] - S[B - 1]
        if d == 0:
            continue
        if out:
            first, gap, step, n = out[-1]
            if step == d and (n == 1 or B == first + n * gap):
                out[-1] = (first, B - first if n == 1 else gap, step, n + 1)
                continue
        out.append((B, 0, d, 1))
    return out


def test_wgrad_workspace_sizes(built):
    """cf_wgrad_ws_bytes / cf_step_wgrads_ws_bytes for every batch 0..8192, exactly: pins wgrad_splits at its 512-workgroup target
    and the skinny 1x1 kernel's split rule at every batch.  NOT pinned here: the Winograd form's split count (256 workgroups to aim
    for) - the workspace is sized for the direct form's, which is never smaller; the GPU digests of tests/test_gpu_parity.py pin it
    at their batches."""
    import hashlib
    from contextflow_amd.layers import _hip
    L = _hip.lib()
    h = hashlib.sha256()
    for shape in WGRAD_WS_SHAPES:
        H, MR, NR, taps = shape
        v = [L.cf_wgrad_ws_bytes(B, MR, NR, H, H, taps) for B in range(8193)]
        for x in v:
            h.update(str(x).encode())
        if shape in WGRAD_WS_RUNS:
            per = 4 * (taps * MR * NR + MR)
            assert all(x % per == 0 for x in v) and v[0] == per, shape
            assert _runs([x // per for x in v]) == WGRAD_WS_RUNS[shape], shape
    assert h.hexdigest() == WGRAD_WS_SHA
    h = hashlib.sha256()
    for C, H, W in SHAPES:
        for B in range(8193):
            h.update(str(L.cf_step_wgrads_ws_bytes(B, C, H, W)).encode())
    assert h.hexdigest() == WGRAD_STEP_WS_SHA


# ---- the mixture launch plan as the size queries see it ---------------------------------------------------------------------------
# Recorded from the library as it was BEFORE cf_gmm.hip got its one gmm_plan (commit bbf7a47).  M K x D: the component tiles (16 |
# 80 wide, ragged, more than 256 components) x widths below one chunk pair, ragged, not a multiple of 4, and the flows' levels.
GMM_WS_MK = (16, 40, 80, 160, 264)                        # K = 8
GMM_WS_D = (48, 64, 96, 99, 100, 768, 1536, 3072)
GMM_WS_LEVELS = ((1536, 768, 768), (2048,), (1024, 1024))  # cifar10; mnist as preset and with split priors
GMM_WS_SHA = "51099e5ed70a874abf875cebea92b6b42471e3ff4ccc6bc143b8e0448a561750"


def test_gmm_workspace_sizes(built):
    """cf_gmm_ws_bytes, cf_gmm_resp_ws_bytes, cf_gmm_keyed_ws_bytes and cf_gmm_levels_ws_bytes for every batch 0..8192, exactly:
    pins the D split of gmm_plan (512 workgroups to aim for, slices of at least one 32-column chunk, at most 64) as each of the
    four queries reports it.  The keyed query runs over T = 1..64 tiles as B advances and once more, all 64, at B = 8192."""
    import ctypes
    import hashlib
    from contextflow_amd.layers import _hip
    L = _hip.lib()
    arr = lambda v: (ctypes.c_int * len(v))(*v)
    levels = [arr(v) for v in GMM_WS_LEVELS]
    h = hashlib.sha256()
    for MK in GMM_WS_MK:
        M, K = MK // 8, 8
        for D in GMM_WS_D:
            for B in range(8193):
                h.update(("%d %d %d " % (L.cf_gmm_ws_bytes(B, M, K, D), L.cf_gmm_resp_ws_bytes(B, M, K, D),
                                         L.cf_gmm_keyed_ws_bytes(1 + B % 64, B, M, K, D))).encode())
            for T in range(1, 65):
                h.update(("%d " % L.cf_gmm_keyed_ws_bytes(T, 8192, M, K, D)).encode())
        for B in range(8193):
            for v in levels:
                h.update(("%d " % L.cf_gmm_levels_ws_bytes(len(v), v, B, M, K)).encode())
    assert h.hexdigest() == GMM_WS_SHA
    five = arr([64] * 5)
    assert L.cf_gmm_levels_ws_bytes(0, five, 256, 10, 8) == -1 and L.cf_gmm_levels_ws_bytes(5, five, 256, 10, 8) == -1
    # the one-level queries report the split count before the slices are rounded to 32 columns, the levels query the launched one
    assert L.cf_gmm_ws_bytes(70, 10, 8, 768) == 16 * 70 * 80 * 4 and L.cf_gmm_levels_ws_bytes(1, arr([768]), 70, 10, 8) == 12 * 70 * 80 * 4


WGRAD_MACS_SCRIPT = """
import sys
sys.path.insert(0, %r)
from contextflow_amd.layers import _hip
L = _hip.lib()
print([L.cf_step_wgrads_macs(B, C, H, W) // (C * C * H * W) for C, H, W in %r for B in (1, 256, 8192)])
"""


@pytest.mark.parametrize("setting,want", [("", [20, 20, 20, 20, 40]), ("CONTEXTFLOW_DIRECT_CONV=1", [40] * 5)])
def test_step_wgrads_macs(built, setting, want):
    """cf_step_wgrads_macs in units of C^2 HW: the 3x3 in the Winograd form (16 of 36) everywhere but at C = 64 on 16x16 (128
    columns keep the direct form), and nowhere under CONTEXTFLOW_DIRECT_CONV=1 (a child process: the switch is read once)."""
    import ast
    env = {k: v for k, v in os.environ.items() if not k.startswith("CONTEXTFLOW_")}
    if setting:
        env.update([setting.split("=")])
    shapes = SHAPES + ((64, 16, 16),)
    r = subprocess.run([sys.executable, "-c", WGRAD_MACS_SCRIPT % (ROOT, shapes)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert ast.literal_eval(r.stdout.strip()) == [w for w in want for _ in range(3)]


def test_gfx950_code_object(built):
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", built], capture_output=True, text=True)
    blob = out.stdout + out.stderr
    assert "gfx950" in blob, blob[:500]


@pytest.mark.parametrize("name", ["mnist", "cifar10", "smap"])
def test_state_dict_matches_reference_layout(name):
    """create_model reproduces the reference's state_dict names/shapes (oracle.params.param_spec is
    itself asserted equal to the real reference state_dict in tests/golden/make_golden.py)."""
    import contextflow_amd as cfa
    from oracle import flow_oracle as fo, params as op
    cfg, data_size, M = cfa.preset_config(name)
    model = cfa.create_model(cfg, data_size, M)
    ops, prior, M2 = fo.program(name)
    spec = op.param_spec(ops, prior, M2)
    sd = model.state_dict()
    assert list(sd.keys()) == list(spec.keys())
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(spec[k][0]), k
    model.load_state_dict(op.gen_params(spec, 0), strict=True)
    n = sum(p.numel() for p in model.parameters())
    assert n == {"mnist": 415360, "cifar10": 1518896, "smap": 936008}[name]


def test_layer_types_follow_program():
    import contextflow_amd as cfa
    from oracle import flow_oracle as fo
    kinds = {"dequant": "Dequantization", "affine": "Normalization", "logit": "LogitTransform", "augment": "Augment",
             "squeeze": "Squeeze", "conv1x1": "Conv1x1", "actnorm": "ActNorm", "coupling": "Coupling",
             "transcoupling": "TransCoupling", "split": "SplitPrior"}
    for name in ("mnist", "cifar10", "smap"):
        cfg, data_size, M = cfa.preset_config(name)
        model = cfa.create_model(cfg, data_size, M)
        ops, _, _ = fo.program(name)
        assert [type(m).__name__ for m in model.sequence_modules] == [kinds[o[0]] for o in ops]


def test_no_cpu_fallback():
    """The product path must fail loudly off-device; the oracle is never imported by the package."""
    import contextflow_amd as cfa
    cfg, data_size, M = cfa.preset_config("mnist")
    model = cfa.create_model(cfg, data_size, M)
    with pytest.raises(RuntimeError, match="ROCm device"):
        model(torch.zeros(2, 1, 32, 32))
    with pytest.raises(RuntimeError, match="ROCm device"):
        cfa.layers.Coupling(8, (3, 3), (1, 1))(torch.zeros(1, 8, 4, 4))
    for root, _, files in os.walk(os.path.join(ROOT, "contextflow_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "/root/reference" not in src, f


def test_unbuilt_names_raise_and_specialist_layout():
    """Names outside the built scope raise at construction; the specialist models that ARE built (eye | onehot +
    uniform context encoders, conv couplings) have the reference's state_dict layout (oracle.params.param_spec is
    checked key for key against the reference by tests/golden/make_golden_specialist.py)."""
    import contextflow_amd as cfa
    from oracle import flow_oracle as fo, params as op
    from tests.helpers import SPECIALIST
    L = cfa.layers
    with pytest.raises(NotImplementedError):
        L.MaskedCoupling(4, context_net=object())
    assert set(L.MaskedCoupling(4, (3, 3), (1, 1)).state_dict()) == {
        "NN.conv%d.%s" % (i, k) for i in (1, 2, 3) for k in ("weight", "bias", "mask")}
    with pytest.raises(NotImplementedError):
        L.ContextEncoder([64], "eye", "vardeq", (16,))          # odd code width: the reference's Augment path
    assert set(L.SplineActivation((2, 2, 2), individual_weights=True).state_dict()) == {
        "unnormalized_widths", "unnormalized_heights", "unnormalized_derivatives"}
    for fxname, (name, ctx) in SPECIALIST.items():
        cfg, ds, M = cfa.preset_config(name)
        cfg.update(generalist=False, enc_emb=ctx["enc_emb"], enc_type=ctx.get("enc_type", "uniform"), contextflow=ctx["contextflow"])
        sd = cfa.create_model(cfg, ds, M, contexts=ctx["contexts"]).state_dict()
        ops, ps, MM = fo.program(name)
        spec = op.param_spec(ops, ps, MM, ctx)
        assert list(sd.keys()) == list(spec.keys()), fxname
        assert all(tuple(sd[k].shape) == tuple(spec[k][0]) for k in sd), fxname


def test_specialist_front_end_takes_uniform_encoders_only():
    """layers/specialist.py::_front_end forms a context code inside cf_linear_group only for encoders whose code IS the uniform
    dequantisation of the one-hot code / of the context itself (model.py:32-49, dequantize.py:26-70); flow-type encoders (vardeq,
    argmax, probsample: the noise comes from a conditional flow) keep their own path.  Host logic only - no kernel runs here."""
    import contextflow_amd as cfa
    from contextflow_amd.layers import specialist
    from contextflow_amd.layers.context import OneHotEncoder, EyeEncoder
    cfg, ds, M = cfa.preset_config("mnist")
    for emb, typ, want in (("onehot", "uniform", 1), ("eye", "uniform", 0), ("onehot", "vardeq", None), ("eye", "argmax", None)):
        contexts = [4, 6] if typ != "argmax" else [4, 16]
        cfg.update(generalist=False, enc_emb=emb, enc_type=typ, contextflow=True)
        flow = cfa.create_model(cfg, ds, M, contexts=contexts)
        assert specialist.supported(flow)
        nets = [m.context_net for m in flow.sequence_modules if getattr(m, "context_net", None)]
        assert nets
        for net in nets:
            got = specialist._uniform_encoder(net)
            if want is None:
                assert got is None, (emb, typ)
            else:
                enc, card, onehot = got
                assert onehot == want and enc is net[1] and isinstance(net[0], OneHotEncoder if want else EyeEncoder)
                assert (card is None) == (want == 0) and enc.D == (sum(contexts) if want else len(contexts)) and net.contexts == contexts
        # without a context (or with the switch off) the front end has nothing to do
        assert specialist._front_end(flow, None, 4, "cpu") == {}


def test_specialist_tape_records_and_their_backwards():
    """layers/_tape.py: every record class has a kind of its own, and the specialist backward (autograd_ctx.BACKWARD, keyed by
    kind) covers exactly the records the specialist training forward appends (autograd_ctx.RECORDS).  Host logic only."""
    from contextflow_amd.layers import _tape, autograd_ctx
    classes = [c for c in vars(_tape).values() if isinstance(c, type) and issubclass(c, tuple) and hasattr(c, "kind")]
    kinds = [c.kind for c in classes]
    assert len(classes) >= 12 and len(set(kinds)) == len(kinds), kinds
    assert len(set(autograd_ctx.RECORDS)) == len(autograd_ctx.RECORDS) and all(r in classes for r in autograd_ctx.RECORDS)
    assert {r.kind for r in autograd_ctx.RECORDS} == set(autograd_ctx.BACKWARD)
    assert all(fn is None or callable(fn) for fn in autograd_ctx.BACKWARD.values())


def test_shard_bounds():
    from contextflow_amd.dist import shard_bounds
    for total in (0, 1, 7, 64, 65536 + 3):
        for world in (1, 2, 3, 8):
            cuts = [shard_bounds(total, r, world) for r in range(world)]
            assert cuts[0][0] == 0 and cuts[-1][1] == total
            assert all(cuts[i][1] == cuts[i + 1][0] for i in range(world - 1))
            sizes = [hi - lo for lo, hi in cuts]
            assert max(sizes) - min(sizes) <= 1


WORKER = r'''
import os, sys, math, torch
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from contextflow_amd.dist import init_process_group, shard_bounds, allreduce_nll, mean_bits_per_dim
from oracle import flow_oracle as fo
from tests.helpers import load_e2e, e2e_inputs
rank, _, world = init_process_group("gloo")
ops, _, M, params, fx = load_e2e("mnist")
x, u, eps = e2e_inputs("mnist", fx)
lo, hi = shard_bounds(x.shape[0], rank, world)
_, logp = fo.flow_forward(ops, params, x[lo:hi], u[lo:hi], [e[lo:hi] for e in eps])   # oracle stands in for the GPU kernels
red = allreduce_nll(torch.logsumexp(logp.double(), -1).sum(), hi - lo)
full = torch.logsumexp(torch.from_numpy(fx["logp"]).double(), -1)
assert int(red[1]) == x.shape[0]
assert abs(float(red[0]) - float(full.sum())) < 1e-2 * x.shape[0], (float(red[0]), float(full.sum()))
bpd = mean_bits_per_dim(red, 1024)
ref = float(-(full.mean()) / (1024 * math.log(2)))
assert abs(bpd - ref) < 1e-5, (bpd, ref)
dist.barrier()
if rank == 0: print("OK", bpd)
'''


def test_two_rank_nll_allreduce_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", WORLD_SIZE="2", OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert "OK" in outs[0]


GRAD_WORKER = r'''
import os, sys, torch
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from contextflow_amd.dist import init_process_group, allreduce_gradients
rank, _, world = init_process_group("gloo")
torch.manual_seed(0)
m = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
for i, p in enumerate(m.parameters()):
    p.grad = torch.full_like(p, float(rank + 1) * (i + 1))
allreduce_gradients(m, bucket_bytes=64)           # tiny buckets: several messages
for i, p in enumerate(m.parameters()):
    assert torch.allclose(p.grad, torch.full_like(p, 1.5 * (i + 1))), (rank, i, p.grad.flatten()[:3])
dist.barrier()
if rank == 0: print("OK")
'''


def test_two_rank_gradient_allreduce_gloo(tmp_path):
    script = tmp_path / "gworker.py"
    script.write_text(GRAD_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29543", WORLD_SIZE="2", OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert "OK" in outs[0]


INIT_WORKER = r'''
import os, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from contextflow_amd.dist import init_process_group, shard_bounds, allreduce_actnorm_sums, broadcast_parameters
rank, _, world = init_process_group("gloo")
fx = np.load(os.path.join(sys.argv[1], "tests", "golden", "unit_layers.npz"))
x = torch.from_numpy(fx["actnorm/x"]).double()              # the reference's first (initialising) batch, (5, 7, 3, 4)
lo, hi = shard_bounds(x.shape[0], rank, world)              # ragged shards: 3 + 2 samples
xs = x[lo:hi]
C = x.shape[1]
# what cf_actnorm_sums leaves on each rank (fp64 per-channel sums of ITS shard), here with torch standing in for the kernel
sums = torch.cat([xs.sum((0, 2, 3)), (xs * xs).sum((0, 2, 3)), torch.tensor([float(xs.shape[0] * 12)], dtype=torch.float64)])
allreduce_actnorm_sums(sums)
n = float(sums[2 * C])
assert n == 5 * 12
mean = sums[:C] / n                                           # cf_actnorm_from_sums (actnorm.py:31-33)
var = ((sums[C:2 * C] - sums[:C] * mean) / (n - 1.0)).clamp_min(0)
logs = torch.log(var.sqrt() + 1e-8)
assert torch.allclose(mean.float(), torch.from_numpy(fx["actnorm/sd:NN_t"]), rtol=1e-6, atol=1e-7), rank
assert torch.allclose(logs.float(), torch.from_numpy(fx["actnorm/sd:NN_logs"]), rtol=1e-6, atol=1e-7), rank

# bucketed parameter broadcast: fp32 parameters + an int64 buffer, rank 1 starts from different values
torch.manual_seed(rank)
m = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.BatchNorm1d(5), torch.nn.Linear(5, 3))
m[1].num_batches_tracked.fill_(40 + rank)
versions = [p._version for p in m.parameters()]
broadcast_parameters(m, src=0)
torch.manual_seed(0)
ref = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.BatchNorm1d(5), torch.nn.Linear(5, 3))
for a, b in zip(m.parameters(), ref.parameters()):
    assert torch.equal(a, b), rank
assert int(m[1].num_batches_tracked) == 40
assert all(p._version > v for p, v in zip(m.parameters(), versions))     # parameter-derived caches key on the version
dist.barrier()
if rank == 0: print("OK")
'''


def test_two_rank_sharded_actnorm_init_and_bucketed_broadcast_gloo(tmp_path):
    """rank-sharded ActNorm init (all-reduce of per-channel sum x, sum x^2, count) equals the
    global-batch init of the reference's fixture; parameters travel as one flat message per dtype."""
    script = tmp_path / "iworker.py"
    script.write_text(INIT_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29545", WORLD_SIZE="2", OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert "OK" in outs[0]


BUCKET_WORKER = r'''
import os, sys, torch
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from contextflow_amd.dist import init_process_group, GradBucket
rank, _, world = init_process_group("gloo")
torch.manual_seed(0)
ps = [torch.nn.Parameter(torch.zeros(*sh)) for sh in ((3, 5), (7,), (2, 2, 3, 3), (1,), (6, 1))]
b = GradBucket([ps[:2], ps[2:4], ps[4:]], torch.device("cpu"))
assert len(b.segments) == 3 and b.flat.numel() == 16 + 8 + 36 + 4 + 8
for i, p in enumerate(ps):                                 # the "gradient kernels" write the views; p.grad IS the view
    b.view(p).fill_(float((rank + 1) * (i + 1)))
    p.grad = b.view(p)
    assert p.grad.data_ptr() == b.flat.data_ptr() + 4 * b.slots[p][0] and p.grad.shape == p.shape
for i in range(len(b.segments)):
    b.reduce(i)                                            # one message per segment, enqueued as soon as it is complete
b.finish()
for i, p in enumerate(ps):
    assert torch.equal(p.grad, torch.full_like(p, 1.5 * (i + 1))), (rank, i, p.grad.flatten()[:3])      # mean over the two ranks
assert b.message_bytes() == [96, 160, 32]
dist.barrier()
if rank == 0: print("OK")
'''


def test_two_rank_gradient_bucket_gloo(tmp_path):
    """dist.GradBucket: p.grad are views of ONE flat tensor, every segment is reduced in place (no cat / copy back), the
    result is the mean over the ranks."""
    script = tmp_path / "bworker.py"
    script.write_text(BUCKET_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", WORLD_SIZE="2", OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert "OK" in outs[0]


@pytest.mark.parametrize("name", ["cifar10", "mnist", "smap"])
def test_gradient_bucket_follows_the_backward(built, name):
    """layers/autograd.py::_bucket_for on the tape the fused plan of a flow would leave (built on the CPU from the plan:
    records carry modules only): every trainable tensor has exactly one slot, slots appear in the order the backward
    produces the gradients (final prior and last level first), a segment closes at every SplitPrior and once it holds
    1 MB, and `closes` names the record after which each segment is complete."""
    import contextflow_amd as cfa
    from contextflow_amd.layers import autograd as ag
    cfg, ds, M = cfa.preset_config(name)
    flow = cfa.create_model(cfg, ds, M)
    for m in flow.modules():
        if hasattr(m, "initialized"):
            m.initialized.fill_(1)
            m._init_done = True
    plan = flow._build_plan(tuple(ds))
    from contextflow_amd.layers import _tape
    tape = []
    for op in plan:
        if op[0] == "pre":
            tape.append(_tape.Pre())
        elif op[0] == "step":
            tape.append(_tape.Step(conv=op[1], act=op[2], cpl=op[3], shape=op[4], squeeze=op[5]))
        elif op[0] == "vstep":
            tape.append(_tape.VStep(conv=op[1], act=op[2], cpl=op[3]))
        elif op[0] == "split":
            tape.append(_tape.Split(dist=op[1].dist))
        elif op[0] == "squeeze":
            tape.append(_tape.Squeeze(p=tuple(op[1].p)))
        else:
            tape.append(_tape.Layer(module=op[1]))
    tape.append(_tape.Prior(dist=flow.dist))
    params = [p for p in flow.parameters() if p.requires_grad]
    b = ag._bucket_for(flow, tape, params)
    assert set(b.slots) == set(params) and len(b.slots) == len(params)
    lo_prev = -1
    order = [p for ri in range(len(tape) - 1, -1, -1) for p in ag._record_params(tape[ri])]
    for p in order:                                         # backward order, 16-byte aligned, disjoint
        lo, n = b.slots[p]
        assert lo > lo_prev and lo % 4 == 0 and n == p.numel()
        lo_prev = lo + n - 1
    assert b.segments[0][0] == 0 and all(a[1] == c[0] for a, c in zip(b.segments, b.segments[1:])) and b.segments[-1][1] == b.flat.numel()
    assert b.segment_of(flow.dist.mG) == 0                 # the final prior leads the first message
    nsplit = sum(1 for r in tape if r.kind == "split")
    assert len(b.segments) >= nsplit + 1
    closed = sorted(i for v in b.closes.values() for i in v)
    assert closed == list(range(len(b.segments)))
    for ri, segs in b.closes.items():                       # the closing record owns the last slot of its segments
        last = max(b.slots[p][0] for p in ag._record_params(tape[ri]))
        assert b.segments[segs[-1]][0] <= last < b.segments[segs[-1]][1]
    if name == "cifar10":
        mb = [v / 2 ** 20 for v in b.message_bytes()]
        assert abs(sum(mb) - 1518896 * 4 / 2 ** 20) < 0.01 and max(mb) < 2.6, mb
    assert ag._bucket_for(flow, tape, params) is b          # kept: p.grad keeps viewing the same storage


def _steps(shape, n):
    """n fused steps of one resolution level: the first with its Squeeze folded in."""
    return [("step", shape, True)] + [("step", shape, False)] * (n - 1)


# The fused plan of every preset as FlowSequential._build_plan grouped it before layers/flowsequential.py was split into
# flowsequential.py / inverse.py / graphs.py: kind per op, with (C, H, W) and the squeeze flag of a conv step, (C, H, W) of a
# transformer step.  The last entry: modules in the pre-processing group at index 0 (None: no such group).
FUSED_PLANS = {
    "cifar10": ([("pre",)] + _steps((16, 16, 16), 4) + [("split",)] + _steps((32, 8, 8), 4) + [("split",)] + _steps((64, 4, 4), 4), 5),
    "mnist": ([("pre",)] + _steps((8, 16, 16), 2) + _steps((32, 8, 8), 2), 5),         # (1 + 1) * 4 = 8 channels: an Augment, as cifar10
    "smap": ([("layer",)] + [("vstep", (26, 8, 1))] * 8, None),
    "msl": ([("layer",)] * 25, None),
    "smd": ([("layer",)] * 24, None),
    "atm": (([("squeeze",)] + [("layer",)] * 16 + [("split",)]) * 2 + [("squeeze",)] + [("layer",)] * 16, None),
}


@pytest.mark.parametrize("name", sorted(FUSED_PLANS))
def test_fused_plan_of_every_preset(built, name):
    """The plan of each preset is the recorded one, op for op, and `preprocessing_group` finds the image flows' group - with
    their Augment - at index 0 and nothing in the time-series flows.  Host only: no kernel is launched."""
    import contextflow_amd as cfa
    from contextflow_amd.layers.dequantize import preprocessing_group
    cfg, ds, M = cfa.preset_config(name)
    flow = cfa.create_model(cfg, ds, M)
    want, group = FUSED_PLANS[name]
    got = []
    for op in flow._build_plan(tuple(ds)):
        got.append((op[0],) + ((tuple(op[4]), bool(op[5])) if op[0] == "step" else (tuple(op[4]),) if op[0] == "vstep" else ()))
    assert got == want
    g = preprocessing_group(flow.sequence_modules)
    if group is None:
        assert g is None
    else:
        mods = flow.sequence_modules
        assert g.count == group and (g.deq, g.n1, g.n2, g.logit) == tuple(mods[:4]) and g.aug is mods[4]
        assert preprocessing_group(mods, 1) is None and preprocessing_group(mods, len(mods) - 2) is None


def test_calls_run_on_the_device_that_owns_the_tensors(built, monkeypatch):
    """`_hip.call` launches on the device the tensor arguments live on, on that device's current stream - the reference
    picks `cuda:N` without torch.cuda.set_device (model.py:170).  Host-side check of the selection logic with stand-in
    tensors (a one-GPU box cannot show a second device): a recording entry point replaces the library."""
    import contextlib
    import ctypes
    import types
    from contextflow_amd.layers import _hip

    def fake(index):
        t = types.SimpleNamespace(device=torch.device("cuda", index))
        ptr = _hip._Ptr(0x1000 * (index + 1))
        ptr._keep = t
        return ptr

    log = []

    class FakeLib:
        def cf_probe(self, *args):
            log.append(("launch", state["current"], [a.value for a in args if isinstance(a, _hip._Stream)]))
            return 0

    state = {"current": 0}

    @contextlib.contextmanager
    def device_ctx(dev):
        prev, state["current"] = state["current"], dev.index
        log.append(("enter", dev.index))
        try:
            yield
        finally:
            state["current"] = prev
            log.append(("exit", dev.index))

    monkeypatch.setattr(_hip, "lib", lambda: FakeLib())
    monkeypatch.setattr(_hip, "_current_device", lambda: state["current"])
    monkeypatch.setattr(_hip, "_device_ctx", device_ctx)
    monkeypatch.setattr(_hip, "_current_stream", lambda dev: types.SimpleNamespace(cuda_stream=0xABC0 + dev.index))
    st0 = _hip._Stream(0xABC0)                       # what `_hip.stream()` returned under the current device 0

    _hip.call("cf_probe", fake(0), fake(0), 7, st0)  # tensors on the current device: no guard, the stream as passed
    assert log == [("launch", 0, [0xABC0])]
    del log[:]
    _hip.call("cf_probe", fake(3), None, fake(3), st0)   # tensors on cuda:3 while cuda:0 is current
    assert log == [("enter", 3), ("launch", 3, [0xABC3]), ("exit", 3)], log
    assert state["current"] == 0
    with pytest.raises(RuntimeError, match="different devices"):
        _hip.call("cf_probe", fake(0), fake(1), st0)
    assert _hip.device_of([3, None, ctypes.c_void_p(5)]) is None      # host-only entry points: nothing to select
    cpu, cuda = torch.zeros(1), types.SimpleNamespace(is_cuda=True, device=torch.device("cuda", 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        _hip.require_device(cpu)
    with pytest.raises(RuntimeError, match="different devices"):
        _hip.require_device(cuda, types.SimpleNamespace(is_cuda=True, device=torch.device("cuda", 0)))


def test_no_library_gemm_in_the_product():
    """Every contraction of the product path is a hand-written kernel reached through the C ABI: no torch matmul."""
    import glob
    pat = re.compile(r"(\s@\s|torch\.(matmul|mm|bmm|einsum|addmm|baddbmm)\b|F\.linear\b|\.matmul\()")
    offenders = []
    for f in glob.glob(os.path.join(ROOT, "contextflow_amd", "**", "*.py"), recursive=True):
        for i, line in enumerate(open(f), 1):
            code = line.split("#", 1)[0]
            if pat.search(code):
                offenders.append("%s:%d: %s" % (os.path.relpath(f, ROOT), i, line.strip()))
    assert not offenders, "\n".join(offenders)
