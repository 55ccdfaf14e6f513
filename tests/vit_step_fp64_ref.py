"""CPU side of tests/test_vit_step_backward_fp64.py: the cases, their inputs, and one transformer flow step (Conv1x1 -> ActNorm ->
TransCoupling at SMAP geometry: C = 26 on 8 x 1 windows, patch (2, 1), dim 52, one head of 64, 4 tokens per sample) as a plain
torch function with `depth` as an argument - oracle/flow_oracle.py hard-wires six layers in vit_dims, so the layer loop is
written here, the same arithmetic as fo.vit_net; the front end and the affine map are the oracle's own functions.

The floor of a tensor is the larger of two fp32 evaluations of this function on the CPU against its fp64 run: as written, and
with the 52 residual-stream features (and the matching rows / columns of every parameter) permuted by a fixed permutation and
permuted back at the end - the same mathematics, another association of every 52-wide sum.

Nothing here touches a GPU: tests/test_vit_step_backward_fp64.py::test_reference_* run it on the CPU."""
from typing import NamedTuple

import torch
import torch.nn.functional as F

from oracle import flow_oracle as fo
from tests.helpers import unit
from tests.step_fp64_ref import rel_err, bar, GRAD_CAP, GRAD_MIN, FLOOR_FACTOR        # noqa: F401  (one set of constants)

SZ, PATCH = (26, 8, 1), (2, 1)
C, HW, DIM, PD, NTOK, HEAD = 26, 8, 52, 26, 4, 64
Q = "NN.0."                                  # the ViT inside TransCoupling.NN (state-dict prefix)
AFFINE = ("Conv1x1.NN", "ActNorm.NN_t", "ActNorm.NN_logs")
PERM = torch.randperm(DIM, generator=torch.Generator().manual_seed(52))
INV_PERM = torch.argsort(PERM)


class Case(NamedTuple):
    B: int
    depth: int = 6
    fwd_form: str = "rs"     # "rs" | "wave": the forward kernel that writes z, ld and the tape
    taped: int = 1           # 1: the backward starts from the forward's residual-stream tape; 0: xtape = None, it runs the layers again
    sliced: int = 0          # 1: x is the channel slice big[:, :26] of a (B, 52, 8, 1) tensor (batch stride 52 * 8)
    gain: float = 1.0        # factor on the perturbation of the fixture's parameters

    @property
    def id(self):
        return "B%d-d%d-%s-%s%s%s" % (self.B, self.depth, self.fwd_form, "tape" if self.taped else "recompute",
                                      "-slice" if self.sliced else "", "-gain%g" % self.gain if self.gain != 1.0 else "")


def _cases():
    # batch sizes: the smallest that reach each branch.  Row-split forward and the backward: 4 samples per workgroup (B = 1: three
    # padded, 3 / 5: ragged first / second workgroup); wave forward: 32 per workgroup (33: the second holds one sample, T = 256).
    # Grouped weight gradient (rowgemm_plan, rows = 16 / 32 x ceil4(B)): B <= 8 one row range per member, 17 / 37 a few, 261 seventeen
    # (the reduce kernel's unrolled 16 plus one in its tail), 1100 the first suggested batch with more than 64 rows per range.
    out = [Case(B) for B in (1, 3, 5, 17, 37, 261, 1100)]
    out += [Case(B, taped=0) for B in (3, 37)]
    out += [Case(B, fwd_form="wave") for B in (3, 33, 37, 261,
                                               3585)]          # TransCoupling.STEP_RS_MAX_BATCH + 1: the first batch training runs in the wave form
    out += [Case(37, fwd_form="wave", taped=0)]                # the backward tables are packed inside vstep_backward
    for depth in (1, 2, 3):
        for B in (5, 37):
            out += [Case(B, depth), Case(B, depth, taped=0), Case(B, depth, fwd_form="wave")]
    out += [Case(37, sliced=1), Case(5, fwd_form="wave", sliced=1)]
    out += [Case(37, gain=4.0)]
    return out


CASES = _cases()


def vit_names(depth):
    """State-dict names of the ViT parameters of a TransCoupling with `depth` layers, in the order of TransCoupling._flat_params."""
    out = [Q + "to_patch_embedding.%d.%s" % (i, wb) for i in (1, 2, 3) for wb in ("weight", "bias")]
    for l in range(depth):
        a, f = Q + "transformer.layers.%d.0." % l, Q + "transformer.layers.%d.1.net." % l
        out += [a + "norm.weight", a + "norm.bias", a + "to_qkv.weight", a + "to_out.weight",
                f + "0.weight", f + "0.bias", f + "1.weight", f + "1.bias", f + "3.weight", f + "3.bias"]
    return out + [Q + "transformer.norm.weight", Q + "transformer.norm.bias"]


def grad_names(depth):
    return ("gx",) + AFFINE + tuple(vit_names(depth))


def draw(case):
    """fp32 CPU tensors of a case: the `trans_ts` fixture's state dict plus seeded perturbations 0.05 gain randn (as
    test_vit_step_tables_batched_equal_single perturbs it), layers >= depth dropped; Wm = QR + 0.1 randn, t = 0.3 randn, logs =
    0.4 randn (as test_vit_step_kernel draws them); x (`big`: the tensor it is a slice of, or None), gz, gld."""
    B, depth = case.B, case.depth
    g = torch.Generator().manual_seed(7919 * B + 104729 * depth + 31 * int(case.gain) + 2 * case.sliced + (case.fwd_form == "wave"))
    r = lambda *sh: torch.randn(*sh, generator=g)
    _, sd = unit("trans_ts")
    p = {}
    for k in vit_names(depth):
        p[k] = sd[k] + 0.05 * case.gain * r(*sd[k].shape)
    p["Conv1x1.NN"] = torch.linalg.qr(r(C, C))[0] + 0.1 * r(C, C)
    p["ActNorm.NN_t"], p["ActNorm.NN_logs"] = 0.3 * r(C), 0.4 * r(C)
    big = None
    if case.sliced:
        big = r(B, 2 * C, HW, 1)
        x = big[:, :C]
    else:
        x = r(B, C, HW, 1)
    return dict(p=p, x=x, big=big, gz=r(B, C, HW, 1), gld=0.5 + r(B).abs())


class _GeluTanhAdjoint(torch.autograd.Function):
    """Exact (erf) GELU forward whose backward differentiates the tanh approximation (a restated defect)."""
    @staticmethod
    def forward(ctx, a):
        ctx.save_for_backward(a)
        return F.gelu(a)

    @staticmethod
    def backward(ctx, g):
        a, = ctx.saved_tensors
        with torch.enable_grad():
            v = a.detach().requires_grad_()
            d, = torch.autograd.grad(F.gelu(v, approximate="tanh").sum(), v)
        return g * d


def _ln_first_moment_only(x, w, b, eps=1e-5):
    """LayerNorm whose adjoint loses its second-moment term: rstd is a constant on the way back (a restated defect)."""
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(-1, keepdim=True) + eps).rsqrt().detach()
    return (x - mean) * rstd * w + b


def vit_net(x0, p, depth, perm=None, defect=None):
    """fo.vit_net (simple_vit.py:117-127) at SMAP geometry with `depth` layers.  perm: the residual stream is carried with its 52
    features in this order (every parameter indexed to match) and put back at the end.  Returns the conditioner output
    (B, 26, 8, 1) and the residual stream at the depth + 1 layer boundaries, each (B, 4, 52) in the original feature order."""
    B = x0.shape[0]
    P = (lambda t, dim=0: t) if perm is None else (lambda t, dim=0: t.index_select(dim, perm))
    back = (lambda t: t) if perm is None else (lambda t: t.index_select(-1, INV_PERM))
    ln = F.layer_norm if defect != "ln" else (lambda x, shape, w, b: _ln_first_moment_only(x, w, b))
    gelu = F.gelu if defect != "gelu" else _GeluTanhAdjoint.apply
    e = Q + "to_patch_embedding."
    # 'b c (h p1) (w p2) -> b (h w) (p1 p2 c)'
    tok = x0.reshape(B, C // 2, NTOK, 2, 1, 1).permute(0, 2, 4, 3, 5, 1).reshape(B, NTOK, PD)
    tok = ln(tok, (PD,), p[e + "1.weight"], p[e + "1.bias"])
    tok = F.linear(tok, P(p[e + "2.weight"]), P(p[e + "2.bias"]))
    tok = ln(tok, (DIM,), P(p[e + "3.weight"]), P(p[e + "3.bias"]))
    tok = tok + P(fo.posemb_sincos_2d(NTOK, 1, DIM).to(tok.dtype), 1)
    stream = [back(tok)]
    for l in range(depth):
        a, f = Q + "transformer.layers.%d.0." % l, Q + "transformer.layers.%d.1.net." % l
        y = ln(tok, (DIM,), P(p[a + "norm.weight"]), P(p[a + "norm.bias"]))
        qq, kk, vv = F.linear(y, P(p[a + "to_qkv.weight"], 1)).chunk(3, dim=-1)
        att = torch.softmax(torch.matmul(qq, kk.transpose(-1, -2)) * HEAD ** -0.5, dim=-1)
        tok = F.linear(torch.matmul(att, vv), P(p[a + "to_out.weight"])) + tok
        y = ln(tok, (DIM,), P(p[f + "0.weight"]), P(p[f + "0.bias"]))
        y = F.linear(gelu(F.linear(y, P(p[f + "1.weight"], 1), p[f + "1.bias"])), P(p[f + "3.weight"]), P(p[f + "3.bias"]))
        tok = y + tok
        stream.append(back(tok))
    tok = back(ln(tok, (DIM,), P(p[Q + "transformer.norm.weight"]), P(p[Q + "transformer.norm.bias"])))
    # 'b (h w) (p1 p2 c) -> b c (h p1) (w p2)'
    return tok.reshape(B, NTOK, 1, 2, 1, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, HW, 1), stream


def step_ref(d, depth, dtype=torch.float64, grads=True, perm=False, defect=None):
    """One step at `dtype` on the CPU from the tensors of draw(): every input and parameter a leaf.  Loss = (z gz).sum() +
    (ld gld).sum().  perm: the permuted form of vit_net.  defect (test_restated_defects_* only): "ln" | "gelu".  Returns a dict:
    z, ld, stream ((depth + 1, B, 4, 52): the residual stream at the layer boundaries), and with grads: gx and one entry per
    parameter name."""
    lv = lambda t: t.detach().to(dtype).clone().requires_grad_(grads)
    p = {k: lv(v) for k, v in d["p"].items()}
    x = lv(d["x"])
    y, l0 = fo.conv1x1_fwd(x, p["Conv1x1.NN"])
    y, l1 = fo.actnorm_fwd(y, p["ActNorm.NN_t"], p["ActNorm.NN_logs"])
    h, stream = vit_net(y[:, : C // 2], p, depth, PERM if perm else None, defect)
    z, l2 = fo.coupling_apply_fwd(y, h)
    ld = l0 + l1 + l2
    out = dict(z=z.detach(), ld=ld.detach(), stream=torch.stack([s.detach() for s in stream]))
    if grads:
        ((z * d["gz"].to(dtype)).sum() + (ld * d["gld"].to(dtype)).sum()).backward()
        out["gx"] = x.grad
        out.update({k: v.grad for k, v in p.items()})
    return out


def floors(d, depth, ref=None):
    """Per tensor: the error of fp32 torch.autograd on the CPU against the fp64 run (`ref`, computed if not given), as written and
    in the permuted form.  Returns (ref, {name: (plain, permuted)}); the floor is the larger of the two."""
    if ref is None:
        ref = step_ref(d, depth)
    a, b = step_ref(d, depth, dtype=torch.float32), step_ref(d, depth, dtype=torch.float32, perm=True)
    return ref, {k: (rel_err(a[k], ref[k]), rel_err(b[k], ref[k])) for k in grad_names(depth)}


def member_shapes(B, depth):
    """(rows, K, N) of the members of the grouped weight gradient as autograd._vstep_param_part forms them from the planes of
    cf_vit_step_bwd (include/contextflow_hip.h): Bp = B rounded up to 4, 8 Bp position rows, 4 Bp token rows."""
    Bp = (B + 3) // 4 * 4
    R4, P8 = 4 * Bp, 8 * Bp
    out = [(P8, C, C), (R4, PD, DIM)]
    for _ in range(depth):
        out += [(R4, DIM, 192), (R4, HEAD, DIM), (R4, DIM, DIM), (R4, DIM, DIM)]
    return out
