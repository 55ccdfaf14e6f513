"""The issue-stream items of the evaluation step kernels (contextflow_amd/csrc/cf_step_common.h: winograd24_phase2 with
CF_W24_SPREAD).  It reorders instructions and changes no arithmetic.  GPU: cf_flow_step_fwd at the smallest
batches that reach the three headline kernels with a ragged last workgroup (16x16: B = 3; 8x8 and 4x4: B = 2051 - the last
workgroup holds 3 of its 4 / 8 samples), plain and squeeze-folded, against the fp64 oracle under the bars of
tests/test_gpu_parity.py::test_winograd_step_kernel_against_the_oracle, and independence of a sample's result from its place
in the batch.  (Bit identity against a build with the switch off needs a second library: tools/dev/issue_stream_parity.py,
recorded in profiles/issue_stream_parity.txt.)  CPU: the classification of tools/isa_census.py on a hand-written listing."""
import importlib.util
import os

import pytest
import torch

from oracle import flow_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SHAPES = [(16, 16, 3), (32, 8, 2051), (64, 4, 2051)]          # C, H = W, batch


# ------------------------------------------------------------------------------------------------------ CPU
LISTING = """
	.amdhsa_kernel _Z5k_onev
	.end_amdhsa_kernel
	.text
_Z5k_onev:                              ; @_Z5k_onev
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	s_waitcnt lgkmcnt(0)
	v_mov_b32_e32 v0, 0
	v_pk_add_f32 v[2:3], v[2:3], v[4:5]
	ds_read2st64_b32 v[4:5], v1 offset1:2
	s_nop 0
	v_mfma_f32_16x16x4_f32 v[8:11], v0, v4, 0
	v_mfma_f32_16x16x4_f32 v[8:11], v0, v5, v[8:11]
	s_nop 8
	buffer_load_dwordx4 v[12:15], v1, s[0:3], 0 offen
	global_store_dword v1, v0, s[0:1]
	scratch_store_dword off, v0, off
	s_barrier
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel _Z5k_twov
	.end_amdhsa_kernel
	.text
_Z5k_twov:                              ; @_Z5k_twov
	v_add_f32_e32 v0, v0, v1
	s_endpgm
	.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .address_space:  global
        .name:           x
        .offset:         0
    .name:           _Z5k_onev
    .private_segment_fixed_size: 8
    .vgpr_count:     16
    .vgpr_spill_count: 1
  - .agpr_count:     0
    .args:           []
    .name:           _Z5k_twov
    .private_segment_fixed_size: 0
    .vgpr_count:     2
    .vgpr_spill_count: 0
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
...
	.end_amdgpu_metadata
"""


def test_census_counts_by_prefix_and_reads_the_metadata():
    spec = importlib.util.spec_from_file_location("isa_census", os.path.join(ROOT, "tools", "isa_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = mod.census(LISTING)
    assert set(rows) == {"_Z5k_onev", "_Z5k_twov"}
    one = rows["_Z5k_onev"]
    assert (one["v_mfma"], one["v_other"], one["ds"], one["vmem"]) == (2, 2, 1, 2)        # scratch_* is neither buffer_* nor global_*
    assert (one["s_nop"], one["s_waitcnt"], one["s_barrier"]) == (2, 1, 1)
    assert (one["vgprs"], one["spill"], one["private"]) == (16, 1, 8)                     # the argument's .name is not the kernel's
    two = rows["_Z5k_twov"]
    assert (two["v_mfma"], two["v_other"], two["vgprs"], two["spill"], two["private"]) == (0, 1, 2, 0, 0)
    names = mod.demangle(list(rows))
    assert names["_Z5k_onev"] == "k_one" and names["_Z5k_twov"] == "k_two"
    assert "| `k_one` | 2 | 2 | 1 | 2 | 2 | 1 | 1 | 16 | 1 | 8 | 4 |" in mod.table(rows, names, ["k_one"])


# ------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


_cases = {}


def step_case(L, C, H, B):
    """(modules on the device, x, fp64 z, fp64 log-det) of one shape: computed once, shared by the tests, left unchanged"""
    if (C, H) not in _cases:
        W = H
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
        _cases[(C, H)] = ((conv, act, cpl), x, zref, l0 + l1 + l2)
    return _cases[(C, H)]


def production_step(mods, xin, C, H, squeeze):
    """cf_flow_step_prepare + cf_flow_step_fwd, the entry point of the evaluation forward"""
    from contextflow_amd.layers import _hip
    lib = _hip.lib()
    conv, act, cpl = mods
    B, W = xin.shape[0], H
    f, pp = _hip.f32, _hip.p
    ws = torch.empty(lib.cf_flow_step_ws_bytes(C, H, W), device=xin.device, dtype=torch.uint8)
    c1, c2, c3 = cpl.NN[0], cpl.NN[2], cpl.NN[4]
    _hip.call("cf_flow_step_prepare", pp(f(conv.NN.detach())), pp(f(act.NN_t.detach())), pp(f(act.NN_logs.detach())),
              pp(f(c1.weight.detach())), pp(f(c1.bias.detach())), pp(f(c2.weight.detach())), pp(f(c2.bias.detach())),
              pp(f(c3.weight.detach())), pp(f(c3.bias.detach())), pp(ws), C, H, W, _hip.stream())
    z = torch.full((B, C, H, W), float("nan"), device=xin.device)
    ldj = torch.zeros(B, device=xin.device)
    _hip.call("cf_flow_step_fwd", pp(xin), pp(z), pp(ldj), pp(ws), B, C, H, W, C * H * W, int(squeeze), _hip.stream())
    torch.cuda.synchronize()
    return z, ldj


@pytest.mark.gpu
@pytest.mark.parametrize("squeeze", [False, True])
@pytest.mark.parametrize("C,H,B", SHAPES)
def test_headline_step_kernels_against_the_oracle_at_a_ragged_batch(L, C, H, B, squeeze):
    """z to 1e-5 of its scale, the log-det to 1e-5 relative (the bars of test_winograd_step_kernel_against_the_oracle)"""
    mods, x, zref, lref = step_case(L, C, H, B)
    xin = fo.squeeze_inv(x, (2, 2)) if squeeze else x
    z, ldj = production_step(mods, xin.to(DEV).contiguous(), C, H, squeeze)
    scale = max(1.0, zref.abs().max().item())
    ez = (z.cpu().double() - zref).abs().max().item()
    el = ((ldj.cpu().double() - lref).abs() / lref.abs().clamp_min(1.0)).max().item()
    print("C%d %dx%d B=%d squeeze=%d: max |dz| %.2e of scale %.2e, max rel |d log-det| %.2e" % (C, H, H, B, squeeze, ez, scale, el))
    assert ez <= 1e-5 * scale
    assert el <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("squeeze", [False, True])
@pytest.mark.parametrize("C,H,B", SHAPES)
def test_a_sample_gives_the_same_bits_wherever_it_sits_in_the_batch(L, C, H, B, squeeze):
    """The batch reversed: sample i moves to another workgroup, and at 8x8 / 4x4 to another lane and column tile of it (2051 = 3
    mod 4 and mod 8).  A patch read that reached a register before its last reader, or after its first, would mix
    neighbouring samples' values; every sample's z and log-det are equal bit for bit instead."""
    mods, x, _, _ = step_case(L, C, H, B)
    xd = (fo.squeeze_inv(x, (2, 2)) if squeeze else x).to(DEV).contiguous()
    z, ldj = production_step(mods, xd, C, H, squeeze)
    zr, ldjr = production_step(mods, xd.flip(0).contiguous(), C, H, squeeze)
    assert torch.isfinite(z).all() and torch.isfinite(ldj).all()
    assert torch.equal(zr.flip(0), z) and torch.equal(ldjr.flip(0), ldj)
