#!/usr/bin/env python3
"""Rounding of ONE transformer flow step (Conv1x1 -> ActNorm -> TransCoupling, SMAP fixture parameters of step `k`) on 4096
inputs drawn like the step's real input: conditioner output h = [t | raw], z and the log-det from the two one-kernel forms
and from the fp32 oracle (= the reference's arithmetic), each against the fp64 oracle - rms and max error relative to the
largest entry.  CONTEXTFLOW_HIP_LIB selects an A/B build.  usage: vit_step_error.py [k=0] [tag=none|stress|extreme]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from tests.gpu_util import build_model, set_noise
from tests.helpers import load_e2e
import oracle.flow_oracle as fo
from contextflow_amd.layers.coupling import TransCoupling

DEV = "cuda:0"
k = int(sys.argv[1]) if len(sys.argv) > 1 else 0
tag = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "none" else None
ops, _, M, params, fx = load_e2e("smap", tag)
B = 4096
g = torch.Generator().manual_seed(3)
x = torch.rand(B, 25, 8, 1, generator=g)
eps = torch.randn(B, 1, 8, 1, generator=g)
p64 = {n: (v.double() if v.is_floating_point() else v) for n, v in params.items()}
tr = []
fo.flow_forward(ops, p64, x.double(), None, [eps.double()], trace=tr)
steps = [i for i, op in enumerate(ops) if op[0] == "transcoupling"]
li = steps[k]                                     # ops[li - 2], ops[li - 1], ops[li] = conv1x1, actnorm, transcoupling
xin = tr[li - 3][2].float() if li >= 3 else None
assert ops[li - 2][0] == "conv1x1" and ops[li - 1][0] == "actnorm"
sz, patch = ops[li][2], ops[li][3]


def oracle(P, xi):
    y, l0 = fo.conv1x1_fwd(xi, P["%d.NN" % ops[li - 2][1]])
    y, l1 = fo.actnorm_fwd(y, P["%d.NN_t" % ops[li - 1][1]], P["%d.NN_logs" % ops[li - 1][1]])
    pre = "%d." % ops[li][1]
    h = fo.vit_net(y[:, : y.shape[1] // 2], P, pre, sz, patch)
    z, l2 = fo.transcoupling_fwd(y, P, pre, sz, patch)
    return h, z, l0 + l1 + l2


h64, z64, l64 = oracle(p64, xin.double())
h32, z32, l32 = oracle(params, xin)
model = build_model("smap", params)
conv, act, cpl = model.sequence_modules[ops[li - 2][1]], model.sequence_modules[ops[li - 1][1]], model.sequence_modules[ops[li][1]]
print("library: %s   step %d of the %s parameter set, |h| <= %.1f, |z| <= %.1f, |ldj| <= %.1f" % (
    os.path.basename(os.environ.get("CONTEXTFLOW_HIP_LIB", "product")), k, tag or "random-init", h64.abs().max(), z64.abs().max(), l64.abs().max()))


def rep(name, h, z, l):
    def e(a, b):
        d = (a.double().cpu() - b).abs()
        return d.pow(2).mean().sqrt().item() / b.abs().max().item(), d.max().item() / b.abs().max().item()
    print("  %-12s h rms %.2e max %.2e | z rms %.2e max %.2e | ldj rms %.2e max %.2e" % ((name,) + e(h, h64) + e(z, z64) + e(l, l64)))


rep("fp32 oracle", h32, z32, l32)
with torch.no_grad():
    for variant in ("wave", "rs"):
        tables = cpl.step_tables([(cpl, conv.NN, act.NN_t, act.NN_logs)], torch.device(DEV), variant)[0]
        ld = torch.zeros(B, device=DEV)
        h = torch.full((B, 26, 8, 1), float("nan"), device=DEV)
        z = cpl.step_forward(xin.to(DEV), tables, ld, h_out=h)
        rep(variant, h, z, ld)
