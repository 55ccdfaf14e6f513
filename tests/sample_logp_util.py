"""Helpers of tests/test_sample_logp.py: the log-density a backward walk returns, restated with the oracle's forward functions.

`walk_logp` is the DEFINITION of `return_logp`: flow_inverse's trace, op by op, and at every recovered input the forward op's
log-det - the split-off halves and the final z scored by gmm_logprob, the channels an Augment drops by std_normal_neg_logq, the
dequantisation noise (the fractional part the floor drops) by log q = 0.  dtype-generic: fp64 in, fp64 out."""
import functools
import math

import torch

from oracle import flow_oracle as fo
from tests.helpers import load_e2e, e2e_inputs

LOG_2PI = math.log(2.0 * math.pi)
BPD_TOL = 1e-5


def cast(params, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params.items()}


def forward_ldj(op, params, xin, zout):
    """The log-det `flow_forward` adds for `op` at its input xin (zout: the op's output, of which an Augment's noise is the tail)."""
    kind, pre = op[0], "%d." % op[1]
    B = xin.shape[0]
    if kind in ("dequant", "squeeze", "permute"):
        return torch.zeros(B, dtype=xin.dtype)
    if kind == "affine":
        return fo.affine_fwd(xin, op[2], op[3])[1]
    if kind == "logit":
        return fo.logit_fwd(xin)[1]
    if kind == "augment":
        return fo.std_normal_neg_logq(zout[:, zout.shape[1] - op[2]:]).reshape(B)      # (B, 1) -> (B,)
    if kind == "conv1x1":
        return fo.conv1x1_fwd(xin, params[pre + "NN"])[1]
    if kind == "actnorm":
        return fo.actnorm_fwd(xin, params[pre + "NN_t"], params[pre + "NN_logs"])[1]
    if kind == "coupling":
        return fo.coupling_fwd(xin, params, pre, op[4])[1]
    if kind == "transcoupling":
        return fo.transcoupling_fwd(xin, params, pre, op[2], op[3])[1]
    if kind == "split":
        h = xin[:, xin.shape[1] // 2:]
        return fo.gmm_logprob(h, params[pre + "dist.mG"], params[pre + "dist.sG"], params[pre + "dist.wG"])
    raise ValueError(kind)


def walk_logp(ops, params, z, halves, records=None):
    """(x, logp (B, M)) of the backward walk from (z, halves); records, if a list, receives (op, recovered input, ldj)."""
    back = []
    x = fo.flow_inverse(ops, params, z, halves, trace=back)
    assert len(back) == len(ops)
    logp = fo.gmm_logprob(z, params["dist.mG"], params["dist.sG"], params["dist.wG"])
    out = z
    for op, (kind, idx, xin) in zip(reversed(ops), back):
        assert (kind, idx) == (op[0], op[1])
        ldj = forward_ldj(op, params, xin, out)
        logp = logp + (ldj if ldj.dim() == 2 else ldj.unsqueeze(-1))
        if records is not None:
            records.append((op, xin, ldj))
        out = xin
    return x, logp


def bpd_entries(logp, D):
    """Every (b, m) entry in bits/dim."""
    return logp.double() / (D * math.log(2.0))


@functools.lru_cache(maxsize=None)
def problem(name, tag=None):
    """The fp64 trace of a committed e2e fixture: (ops, params, z, halves, inputs, logp of flow_forward, D, the ops' log-dets)."""
    ops, _, _, params, fx = load_e2e(name, tag)
    x, u, eps = e2e_inputs(name, fx)
    tr = []
    p64 = cast(params, torch.float64)
    _, logp = fo.flow_forward(ops, p64, x.double(), None if u is None else u.double(), [e.double() for e in eps], trace=tr)
    z, halves, inputs = fo.inverse_problem(ops, x.double(), tr)
    D = 1
    for n in fo.CONFIGS[name][0]:
        D *= int(n)
    return ops, params, z, halves, inputs, logp, D, [t[3] for t in tr]


@functools.lru_cache(maxsize=None)
def floors(name):
    """(walk_logp in fp64, its fp32 run from the fp64 latents, the worst entry of their difference in bits/dim)."""
    ops, params, z, halves, _, _, D, _ = problem(name)
    _, lp64 = walk_logp(ops, cast(params, torch.float64), z, halves)
    _, lp32 = walk_logp(ops, cast(params, torch.float32), z.float(), [h.float() for h in halves])
    assert lp32.dtype == torch.float32
    return lp64, lp32, (bpd_entries(lp32, D) - bpd_entries(lp64, D)).abs().max().item()


def postprocess_ld_closed_form(y, e, t1, s1, t2, s2):
    """ld of cf_postprocess_inv_ld without its ldj_const handed in, in the dtype of y: y (B, n_keep) the kept logits, e (B, aug_n) the
    dropped Augment elements, Normalization 1 / 2 = (t1, s1) / (t2, s2).  -N log s1 - N log s2 + sum softplus(y) + softplus(-y)
    + sum e^2 / 2 + aug_n log(2 pi) / 2."""
    sp = torch.nn.functional.softplus
    N = y.shape[1]
    cst = -N * math.log(s1) - N * math.log(s2)
    return cst + (sp(y) + sp(-y)).sum(-1) + 0.5 * (e * e).sum(-1) + 0.5 * e.shape[1] * LOG_2PI
