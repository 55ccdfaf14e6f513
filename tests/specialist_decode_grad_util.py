"""CPU side of tests/test_specialist_decode_grad.py: the inverse of the specialist Coupling with its per-sample bias restated over
tests/step_fp64_ref.py (the two ReLUs as `a * m`), the cases of the two kernel tests, the fp64 formula of the transposed affine
pair, and the fp64 / fp32 autograd references of the whole backward walk of a specialist fixture (tests/specialist_inverse_util.py
::spec_inverse continued through the oracle's pre-processing, stopped in front of the floor).

Nothing here touches a GPU."""
import functools

import torch
import torch.nn.functional as F

from oracle import flow_oracle as fo
from tests import specialist_inverse_util as SU
from tests import step_fp64_ref as R

# the four geometries, one per level.  VJP kernel (k_flow_step_bwd<.., INV, IB>): (C, H, B) with two or more workgroups and a ragged
# last one at every level (the sizes step_fp64_ref.MODE1 uses for this kernel family) and a single sample; both bias modes; x dense
# and a channel slice of a tensor with twice the channels (batch stride).
GEOMETRIES = [(8, 16, 3), (16, 16, 3), (32, 8, 7), (64, 4, 19)]
# The seeds are those for which the fp64 run has NO ReLU unit inside step_fp64_ref.in_band: the kernel's masks cannot be read back.
_SEEDS = {
    # (C, B, sliced, mode): seed, 0 elsewhere   (searched on the CPU, pinned by test_kernel_inputs_stay_clear_of_the_relu_band)
    (8, 3, 0, 1): 4, (8, 3, 1, 1): 2, (8, 3, 0, 2): 1, (8, 3, 1, 2): 1, (16, 3, 1, 1): 1, (16, 3, 0, 2): 3, (16, 3, 1, 2): 3,
    (16, 1, 0, 1): 1, (16, 1, 1, 1): 1, (64, 19, 0, 1): 1, (64, 19, 1, 1): 1, (64, 19, 0, 2): 2,
}
# forward kernel (k_flow_step_inv<.., CTX>): one geometry per level at every batch size - a single sample, and 37: 37 workgroups at
# 16x16, 10 at 8x8 (4 samples each) and 5 at 4x4 (8 each), the last one ragged at both
FWD_BATCHES = (1, 37)


def _bwd_cases():
    out = []
    for C, H, B in GEOMETRIES:
        for b in (B, 1):
            for mode in (1, 2):
                for sliced in (0, 1):
                    out.append(R.Case(C, H, b, sliced=sliced, mode=mode, seed=_SEEDS.get((C, b, sliced, mode), 0)))
    return out


def _fwd_cases():
    return [R.Case(C, H, b, sliced=sliced, mode=mode) for C, H, _ in GEOMETRIES for b in FWD_BATCHES for mode in (1, 2)
            for sliced in (0, 1)]


BWD_CASES = _bwd_cases()
FWD_CASES = _fwd_cases()
case_id = lambda c: c.id


@functools.lru_cache(maxsize=None)
def drawn(case):
    """(inputs of the case, the true-ReLU fp64 run of the FORWARD coupling): x is the coupling input, ref["z"] the latent its inverse
    starts from, d["gz"] serves as the upstream gradient gx of the inverse (it has the shape of x)."""
    d = R.draw(case)
    return d, R.step_ref(d, mode=case.mode, grads=False)


def coupling_inv_ref(d, z, mode, m1=None, m2=None, dtype=torch.float64, gx=None):
    """The specialist Coupling backwards at `dtype` on the CPU: [tau | raw] = NN(z0) (+) sbias - mode 1 on the conditioner output,
    mode 2 before the first ReLU - s = 2 tanh(raw / 2), x = [z0 | (z1 - tau) e^{-s}].  ReLUs as a * m with m1 / m2 bool, None = the
    true ReLU.  z is a leaf; with gx (the upstream dL/dx) the result carries "gz", the vector-Jacobian product by torch.autograd.
    Returns x, a1, a2 (detached) [, gz]."""
    p = {k: v.detach().to(dtype) for k, v in d["p"].items()}
    sb = d["sbias"].detach().to(dtype)
    z = z.detach().to(dtype).clone().requires_grad_(gx is not None)
    B, C = z.shape[:2]
    a1 = F.conv2d(z[:, : C // 2], p["NN.0.weight"], p["NN.0.bias"])
    if mode == 2:
        a1 = a1 + sb.view(B, -1, 1, 1)
    h1 = a1 * (a1.detach() > 0 if m1 is None else m1).to(dtype)
    a2 = F.conv2d(F.pad(h1, (1, 1, 1, 1), mode="reflect"), p["NN.2.weight"], p["NN.2.bias"])
    h2 = a2 * (a2.detach() > 0 if m2 is None else m2).to(dtype)
    h = F.conv2d(h2, p["NN.4.weight"], p["NN.4.bias"])
    if mode == 1:
        h = h + sb.view(B, -1, 1, 1)
    x = fo.coupling_apply_inv(z, h)
    out = dict(x=x.detach(), a1=a1.detach(), a2=a2.detach())
    if gx is not None:
        (x * gx.to(dtype)).sum().backward()
        out["gz"] = z.grad
    return out


def coupling_inv_floor(d, z, mode, gx, ref_gz):
    """The error of fp32 torch.autograd on the CPU on the same graph (from the fp32 rounding of the same z), against the fp64 run."""
    r32 = coupling_inv_ref(d, z.float(), mode, dtype=torch.float32, gx=gx)
    return R.rel_err(r32["gz"], ref_gz)


def affine_inv_bwd_ref(gx, m1, Wm, m2, logs, dtype=torch.float64):
    """gz = exp(l_b) (W_b^-T gx) per pixel in `dtype` on the CPU: torch.linalg.solve on W_b^T - the formula
    cf_affine_ctx_inv_bwd_data computes.  gx in the (B, C, H, W) layout of z."""
    B, C = gx.shape[:2]
    d = lambda v: None if v is None else v.to(dtype)
    g = d(gx).reshape(B, C, -1)
    if m1 is not None:
        M1 = d(m1).view(B, C, C)
        Wb = torch.tril(M1, -1) + torch.diag_embed(torch.exp(torch.diagonal(M1, dim1=1, dim2=2)))
        if Wm is not None:
            Wb = Wb + d(Wm) - torch.eye(C, dtype=dtype)
        g = torch.linalg.solve(Wb.transpose(1, 2), g)
    if m2 is not None:
        lb = d(m2)[:, C:]
        if logs is not None:
            lb = lb + d(logs)
        g = g * torch.exp(lb)[:, :, None]
    return g.reshape(gx.shape)


# ------------------------------------------------------------------------------------------------ the whole backward walk
# the chain fixtures whose gradient fp32 can hold (mnist_eye_cf: fp32 CPU autograd is itself 6.7e-4 from fp64 there, so no bar
# derived from that floor means anything; it serves the forward value, the pixels and the plumbing)
GRAD_FIXTURES = [f for f in SU.CHAIN_FIXTURES if f != "mnist_eye_cf"]


def _chain(p, dtype):
    """(x, [z, halves...] as leaves): the continuous point of the backward walk of problem p at `dtype`."""
    prm = SU.cast(p.params, dtype)
    code = SU.codes(p.ops, prm, p.ctx, p.context, p.cnoise, dtype)
    lat = [t.detach().to(dtype).clone().requires_grad_(True) for t in [p.z] + list(p.halves)]
    y = SU.spec_inverse(p.ops, prm, p.ctx, code, lat[0], lat[1:], p.first)
    return fo.flow_inverse(p.ops[:p.first], prm, y, stop="dequant"), lat


@functools.lru_cache(maxsize=None)
def chain_reference(fxname, seed=5):
    """(gx, x64, [g_z, g_half...] in fp64, fp32 floor per latent, error of the fp32 forward value in units of max(1, max|x|)) of a
    specialist fixture's trace latents (specialist_inverse_util.problem(fxname, 4)) under a fixed random upstream gx: fp64
    autograd through the restated inverse, and the error fp32 CPU autograd makes on the same graph."""
    p = SU.problem(fxname, 4)
    x64, lat64 = _chain(p, torch.float64)
    gx = torch.randn(x64.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    (x64 * gx).sum().backward()
    x32, lat32 = _chain(p, torch.float32)
    (x32 * gx.float()).sum().backward()
    ref = [t.grad for t in lat64]
    floor = [(a.grad.double() - b).abs().max().item() / b.abs().max().item() for a, b in zip(lat32, ref)]
    return gx, x64.detach(), ref, floor, SU.err_of(x32, x64)
