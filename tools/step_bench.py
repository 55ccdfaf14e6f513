#!/usr/bin/env python3
"""Micro-benchmark of the fused step kernel alone (GPU box).  usage: step_bench.py [B] [flags...] ; prints TFLOP/s per shape
for the default geometry ("base") and for each `flags` value given: bits 16..19 = kernel variant of the test hook
cf_flow_step_fwd_debug (e.g. 0x40000 = variant 4; its table is kDebugKernel in csrc/cf_step.hip: 2 half-size workgroups,
3 k_flow_step_small direct, 4 Winograd F(2x2), 5 row-split 4x4, 6 Winograd F(2x4) at 8x8 and 4x4, 7 the zero-skipping F(2x4) kernel of the 4x4 level); the other bits are unused.  A shape without that variant prints "n/a"."""
import ctypes
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import contextflow_amd as cfa
from contextflow_amd.layers import _hip

L = cfa.layers
B = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
lib = _hip.lib()
fn = lib.cf_flow_step_fwd_debug
fn.restype = ctypes.c_int
fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
FLOP = None
dev = "cuda:0"
variants = [("base", 0)]
for a in sys.argv[2:]:
    variants.append((a, int(a, 0)))
for C, H, W in ((8, 16, 16), (16, 16, 16), (32, 8, 8), (64, 4, 4)):
    torch.manual_seed(0)
    conv, act, cpl = L.Conv1x1((C, H, W)).to(dev), L.ActNorm((C, H, W)).to(dev), L.Coupling(C, (3, 3), (1, 1)).to(dev)
    x = torch.randn(B, C, H, W, device=dev)
    ws = torch.empty(lib.cf_flow_step_ws_bytes(C, H, W), device=dev, dtype=torch.uint8)
    f, pp = _hip.f32, _hip.p
    c1, c2, c3 = cpl.NN[0], cpl.NN[2], cpl.NN[4]
    _hip.call("cf_flow_step_prepare", pp(f(conv.NN.detach())), pp(f(act.NN_t.detach())), pp(f(act.NN_logs.detach())),
              pp(f(c1.weight.detach())), pp(f(c1.bias.detach())), pp(f(c2.weight.detach())), pp(f(c2.bias.detach())),
              pp(f(c3.weight.detach())), pp(f(c3.bias.detach())), pp(ws), C, H, W, _hip.stream())
    z = torch.empty_like(x)
    ldj = torch.zeros(B, device=dev)
    res = []
    for name, flags in variants:
        try:
            for _ in range(3):
                _hip.check(fn(pp(x), pp(z), pp(ldj), pp(ws), B, C, H, W, C * H * W, 0, None, flags, _hip.stream()))
        except RuntimeError:
            res.append("%s: n/a" % name)         # this shape has no such variant
            continue
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20
        e0.record()
        for _ in range(n):
            _hip.check(fn(pp(x), pp(z), pp(ldj), pp(ws), B, C, H, W, C * H * W, 0, None, flags, _hip.stream()))
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / n
        res.append("%s: %.3f ms %.1f TF" % (name, ms, B * 80 * H * W * C * C / ms / 1e9))
    print("C%d B%d | " % (C, B) + " | ".join(res), flush=True)
