"""CPU side of tests/test_vit_decode_grad.py: the inverse of one transformer flow step (TransCoupling^-1 -> ActNorm^-1 ->
Conv1x1^-1) written over tests/vit_step_fp64_ref.py (`vit_net`, with `depth` as an argument) and oracle/flow_oracle.py, the cases
of the kernel test, and the fp64 / fp32 autograd references of the backward walk over the committed smap fixture: each of its
eight steps, two four-step sub-chains and the whole model.

Nothing here touches a GPU."""
import functools

import torch

from oracle import flow_oracle as fo
from tests import vit_step_fp64_ref as V
from tests.sample_logp_util import cast, problem

# depth 1, 2 and the model's 6; B = 1: a quarter-filled workgroup, 5: one full workgroup and one sample, 37: ten workgroups with a
# ragged last one; x dense and - at the batch sizes where a batch stride exists - a channel slice of a tensor with twice the channels
CASES = [V.Case(B, depth, sliced=s) for depth in (1, 2, 6) for B, s in ((1, 0), (5, 0), (5, 1), (37, 0), (37, 1))]
SEED = 3                                                    # of every upstream gradient over the fixture
NSTEPS = 8
SUBCHAINS = {"steps1-4": (1, 13), "steps5-8": (13, 25)}     # op ranges of the smap program: [augment, 8 x (conv1x1, actnorm, transcoupling)]


@functools.lru_cache(maxsize=None)
def drawn(case):
    """(inputs of the case, its fp64 forward run): x is the step input, ref["z"] the latent the inverse starts from, d["gz"]
    serves as the upstream gradient gx of the inverse step (it has the shape of x)."""
    d = V.draw(case)
    return d, V.step_ref(d, case.depth, grads=False)


def vit_step_inv_ref(d, depth, z, dtype=torch.float64, gx=None):
    """One inverse step at `dtype` on the CPU: y0 = z0, [tau | raw] = ViT(z0), s = 2 tanh(raw / 2), y1 = (z1 - tau) e^{-s},
    x = W^-1 (y e^{logs} + t).  z is a leaf; with gx (the upstream dL/dx) the result carries "gz" = the vector-Jacobian product by
    torch.autograd.  Returns a dict: x (detached) [, gz]."""
    p = {k: v.detach().to(dtype) for k, v in d["p"].items()}
    z = z.detach().to(dtype).clone().requires_grad_(gx is not None)
    h, _ = V.vit_net(z[:, : V.C // 2], p, depth)
    y = fo.coupling_apply_inv(z, h)
    x = fo.conv1x1_inv(fo.actnorm_inv(y, p["ActNorm.NN_t"], p["ActNorm.NN_logs"]), p["Conv1x1.NN"])
    out = dict(x=x.detach())
    if gx is not None:
        (x * gx.to(dtype)).sum().backward()
        out["gz"] = z.grad
    return out


def vit_step_inv_floor(d, depth, z, gx, ref_gz):
    """The error of fp32 torch.autograd on the CPU on the same graph (from the fp32 rounding of the same z), against the fp64 run."""
    return V.rel_err(vit_step_inv_ref(d, depth, z.float(), dtype=torch.float32, gx=gx)["gz"], ref_gz)


# ------------------------------------------------------------------------------------------------ the smap fixture
def inverse_reference(ops, params, z, seed=SEED):
    """(gx, x64, gz in fp64, fp32 floor) of the backward walk over `ops` from z under a fixed random upstream gx: fp64 autograd
    through fo.flow_inverse, and the error fp32 CPU autograd makes on the same graph, relative to the largest entry."""
    def run(dtype):
        zz = z.detach().to(dtype).clone().requires_grad_(True)
        return fo.flow_inverse(ops, cast(params, dtype), zz), zz

    x64, z64 = run(torch.float64)
    gx = torch.randn(x64.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    (x64 * gx).sum().backward()
    x32, z32 = run(torch.float32)
    (x32 * gx.float()).sum().backward()
    ref = z64.grad
    floor = (z32.grad.double() - ref).abs().max().item() / ref.abs().max().item()
    return gx, x64.detach(), ref, floor


@functools.lru_cache(maxsize=None)
def smap_range(lo, hi):
    """inverse_reference of ops[lo:hi] of the smap fixture from the traced output of ops[hi - 1], with that latent in front:
    (z, gx, x64, gz, floor)."""
    ops, params, _, _, inputs, _, _, _ = problem("smap")
    z = inputs[hi]
    return (z,) + inverse_reference(ops[lo:hi], params, z)


def smap_step(k):
    """Step k = 0 .. 7 of the smap fixture: ops[1 + 3 k : 4 + 3 k]."""
    return smap_range(1 + 3 * k, 4 + 3 * k)


def smap_whole():
    ops = problem("smap")[0]
    return smap_range(0, len(ops))


def rel(got, ref):
    """max |got - ref| / max |ref|"""
    return (got.detach().cpu().double() - ref).abs().max().item() / ref.abs().max().item()
