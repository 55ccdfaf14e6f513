"""CPU side of tests/test_decode_grad.py: the inverse of one fused conv flow step (Coupling^-1 -> ActNorm^-1 -> Conv1x1^-1) written
over oracle/flow_oracle.py in the style of tests/step_fp64_ref.py::step_ref - the two ReLUs as `a * m`, so that masks can be
imposed - the cases of the kernel test, and the fp64 / fp32 autograd references of the whole backward walk.

Nothing here touches a GPU."""
import functools

import torch
import torch.nn.functional as F

from oracle import flow_oracle as fo
from tests import step_fp64_ref as R
from tests.sample_logp_util import cast, problem

# (C, H, B): two or more workgroups with a ragged last one at every level of k_flow_step_bwd (the sizes step_fp64_ref.MODE1 uses
# for this kernel family), and a single sample; x dense, and a channel slice of a tensor with twice the channels (batch stride).
# The seeds are those for which the fp64 run has NO unit inside step_fp64_ref.in_band: the kernel's masks cannot be read back.
_SEEDS = {
    # (C, B, sliced): seed, 0 elsewhere      (searched on the CPU, pinned by test_kernel_inputs_stay_clear_of_the_relu_band)
    (8, 3, 1): 1, (32, 7, 0): 1, (32, 7, 1): 1, (64, 1, 0): 1, (64, 1, 1): 1,
}
GEOMETRIES = [(8, 16, 3), (16, 16, 3), (32, 8, 7), (64, 4, 19)]


def _cases():
    out = []
    for C, H, B in GEOMETRIES:
        for b in (B, 1):
            for sliced in (0, 1):
                out.append(R.Case(C, H, b, sliced=sliced, seed=_SEEDS.get((C, b, sliced), 0)))
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def drawn(case):
    """(inputs of the case, the true-ReLU fp64 forward run): x is the step input, ref["z"] the latent the inverse starts from,
    d["gz"] serves as the upstream gradient gx of the inverse step (it has the shape of x)."""
    d = R.draw(case)
    return d, R.step_ref(d, grads=False)


def step_inv_ref(d, z, m1=None, m2=None, dtype=torch.float64, gx=None):
    """One inverse step at `dtype` on the CPU: y0 = z0, [tau | raw] = NN(z0), s = 2 tanh(raw / 2), y1 = (z1 - tau) e^{-s},
    x = W^-1 (y e^{logs} + t).  ReLUs as a * m with m1 / m2 (B, 2C, H, W) bool, None = the true ReLU.  z is a leaf; with gx (the
    upstream dL/dx) the result carries "gz" = the vector-Jacobian product by torch.autograd.  Returns x, a1, a2 (detached) [, gz]."""
    p = {k: v.detach().to(dtype) for k, v in d["p"].items()}
    z = z.detach().to(dtype).clone().requires_grad_(gx is not None)
    C = z.shape[1]
    a1 = F.conv2d(z[:, : C // 2], p["NN.0.weight"], p["NN.0.bias"])
    h1 = a1 * (a1.detach() > 0 if m1 is None else m1).to(dtype)
    a2 = F.conv2d(F.pad(h1, (1, 1, 1, 1), mode="reflect"), p["NN.2.weight"], p["NN.2.bias"])
    h2 = a2 * (a2.detach() > 0 if m2 is None else m2).to(dtype)
    h = F.conv2d(h2, p["NN.4.weight"], p["NN.4.bias"])
    y = fo.coupling_apply_inv(z, h)
    x = fo.conv1x1_inv(fo.actnorm_inv(y, p["ActNorm.NN_t"], p["ActNorm.NN_logs"]), p["Conv1x1.NN"])
    out = dict(x=x.detach(), a1=a1.detach(), a2=a2.detach())
    if gx is not None:
        (x * gx.to(dtype)).sum().backward()
        out["gz"] = z.grad
    return out


def step_inv_floor(d, z, gx, ref_gz):
    """The error of fp32 torch.autograd on the CPU on the same graph (from the fp32 rounding of the same z), against the fp64 run."""
    r32 = step_inv_ref(d, z.float(), dtype=torch.float32, gx=gx)
    return R.rel_err(r32["gz"], ref_gz)


# ------------------------------------------------------------------------------------------------ the whole backward walk
def continuous_inverse(ops, params, z, halves):
    """fo.flow_inverse stopped in front of the dequantisation: the tensor floor() would be applied to."""
    return fo.flow_inverse(ops, params, z, halves, stop="dequant")


@functools.lru_cache(maxsize=None)
def chain_reference(name, seed=5):
    """(z, halves, gx, x64, [g_z, g_half...] in fp64, fp32 floor per latent) of a committed fixture's trace latents under a fixed
    random upstream gx: fp64 autograd through the oracle's inverse, and the error fp32 CPU autograd makes on the same graph."""
    ops, params, z, halves, inputs, _, _, _ = problem(name)

    def run(dtype):
        lat = [t.detach().to(dtype).clone().requires_grad_(True) for t in [z] + list(halves)]
        x = continuous_inverse(ops, cast(params, dtype), lat[0], lat[1:])
        return x, lat

    x64, lat64 = run(torch.float64)
    gx = torch.randn(x64.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    (x64 * gx).sum().backward()
    x32, lat32 = run(torch.float32)
    (x32 * gx.float()).sum().backward()
    ref = [t.grad for t in lat64]
    floor = [(a.grad.double() - b).abs().max().item() / b.abs().max().item() for a, b in zip(lat32, ref)]
    return z, list(halves), gx, x64.detach(), ref, floor
