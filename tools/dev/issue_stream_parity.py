#!/usr/bin/env python3
"""Bit identity of the issue-stream items of the evaluation step kernels (GPU box): cf_flow_step_fwd of two library builds on the
same operands, at the smallest batches that reach the three headline kernels with a ragged last workgroup (16x16: B = 3; 8x8 and
4x4: B = 2051), plain and squeeze-folded, and at one large batch (many rounds of workgroups per CU).  z and log-det must be
equal bit for bit.  Both libraries are loaded into this one process.
usage: issue_stream_parity.py LIB_A LIB_B      (a bare tag = contextflow_amd/build/abl/libcf_abl_<tag>.so, 'prod' = the in-tree
library; e.g. `make_abl.py off --only=cf_step.hip -DCF_W24_SPREAD=0` then `issue_stream_parity.py prod off`)"""
import ctypes
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
import torch
import contextflow_amd as cfa
from contextflow_amd.layers import _hip


def load(tag):
    path = _hip.LIB_PATH if tag == "prod" else tag if os.path.sep in tag else os.path.join(root, "contextflow_amd/build/abl/libcf_abl_%s.so" % tag)
    lib = ctypes.CDLL(path)
    for name in ("cf_flow_step_ws_bytes", "cf_flow_step_prepare", "cf_flow_step_fwd"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _hip.SIGNATURES[name]
    return path, lib


def step(lib, mods, x, C, H, W, squeeze):
    conv, act, cpl = mods
    B = x.shape[0]
    f, pp = _hip.f32, _hip.p
    ws = torch.empty(lib.cf_flow_step_ws_bytes(C, H, W), device=x.device, dtype=torch.uint8)
    c1, c2, c3 = cpl.NN[0], cpl.NN[2], cpl.NN[4]
    rc = lib.cf_flow_step_prepare(pp(f(conv.NN.detach())), pp(f(act.NN_t.detach())), pp(f(act.NN_logs.detach())),
                                  pp(f(c1.weight.detach())), pp(f(c1.bias.detach())), pp(f(c2.weight.detach())), pp(f(c2.bias.detach())),
                                  pp(f(c3.weight.detach())), pp(f(c3.bias.detach())), pp(ws), C, H, W, _hip.stream())
    assert rc == 0, rc
    z = torch.full((B, C, H, W), float("nan"), device=x.device)
    ldj = torch.zeros(B, device=x.device)
    rc = lib.cf_flow_step_fwd(pp(x), pp(z), pp(ldj), pp(ws), B, C, H, W, C * H * W, int(squeeze), _hip.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return z, ldj


def main():
    (pa, la), (pb, lb) = load(sys.argv[1]), load(sys.argv[2])
    print("A = %s\nB = %s" % (os.path.relpath(pa, root), os.path.relpath(pb, root)))
    L, dev, bad = cfa.layers, "cuda:0", 0
    for C, H, batches in ((16, 16, (3, 4099)), (32, 8, (2051, 16387)), (64, 4, (2051, 32771))):
        W = H
        torch.manual_seed(C * 1000 + 7)
        mods = (L.Conv1x1((C, H, W)), L.ActNorm((C, H, W)), L.Coupling(C, kernel_size=(3, 3), padding=(1, 1)))
        with torch.no_grad():
            mods[0].NN.add_(0.1 * torch.randn(C, C))
            mods[1].NN_t.copy_(0.3 * torch.randn(C)); mods[1].NN_logs.copy_(0.2 * torch.randn(C))
        for m in mods:
            m.to(dev)
        for B in batches:
            x = torch.randn(B, C, H, W, device=dev)
            for squeeze in (False, True):
                xin = x.reshape(B, C // 4, 2 * H, 2 * W) if squeeze else x       # the kernel folds Squeeze((2,2)) into its loads
                za, la_ = step(la, mods, xin, C, H, W, squeeze)
                zb, lb_ = step(lb, mods, xin, C, H, W, squeeze)
                ok = torch.equal(za, zb) and torch.equal(la_, lb_) and bool(torch.isfinite(za).all())
                bad += not ok
                print("C%-2d %2dx%-2d B=%-6d %-7s z %s  log-det %s  (max |z| %.3f)" % (
                    C, H, W, B, "squeeze" if squeeze else "plain", "equal" if torch.equal(za, zb) else "DIFFERENT",
                    "equal" if torch.equal(la_, lb_) else "DIFFERENT", za.abs().max().item()), flush=True)
    print("parity %s" % ("ok" if not bad else "FAILED: %d cases" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
