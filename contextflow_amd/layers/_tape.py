"""Records of the training tape: FlowSequential._forward_fused writes one per plan group, autograd.FlowLogProb.backward walks
them in reverse and dispatches on `kind` (a class attribute: nothing per record).  Fields that only a training forward on the
device knows default to None, so a tape can be laid out from the modules alone (autograd._bucket_for)."""
from typing import Any, NamedTuple

import torch

from . import _hip


def step_tape(B, C, H, W, dev):
    """Buffers of one step's training tape (cf_flow_step_fwd_taped): y0 (B, C/2, HW), h1, h2 (B, 2C, HW) - the operands of
    the weight-gradient GEMMs - and the opaque aux buffer (log-scales, second half of the Conv1x1+ActNorm output, ReLU
    masks) that is all the step-backward kernel reads of the forward."""
    planes = [torch.empty(B, r, H * W, device=dev, dtype=torch.float32) for r in (C // 2, 2 * C, 2 * C)]
    planes.append(torch.empty(_hip.lib().cf_flow_step_tape_aux_bytes(B, C, H, W), device=dev, dtype=torch.uint8))
    return tuple(planes)


class Pre(NamedTuple):
    """pre-processing: nothing trainable at or above it; its backward (cf_preprocess_bwd, only when the input needs a
    gradient) reads the forward output alone.  The specialist tape (autograd_ctx.taped_forward) also writes it for the time-series
    flows, which have no transform in front ([Augment] alone): y stays None there and the backward is a channel slice; n = 0
    marks a prefix the input gradient is not built for."""
    kind = "pre"
    y: Any = None            # forward output (B, C + aug, H, W): the tensor the next record reads anyway
    n: int = 0               # data elements per sample (the Augment channels behind them get no gradient)
    s1: float = 1.0          # scales of the two Normalizations
    s2: float = 1.0


class Step(NamedTuple):
    """[Squeeze ->] Conv1x1 -> ActNorm -> Coupling in one kernel"""
    kind = "step"
    conv: Any
    act: Any
    cpl: Any
    shape: tuple             # (C, H, W) of the step (behind its Squeeze)
    squeeze: Any             # truthy: x is the tensor in front of the Squeeze
    x: Any = None            # step input
    ws: Any = None           # packed forward tables
    winv: Any = None         # Wm^-1
    planes: Any = None       # step_tape(...) of the forward, or None = rebuilt from x at backward time
    wsb: Any = None          # packed backward tables
    aux: Any = None          # data-only walk (input gradient with frozen weights): the tape's aux buffer, all that is kept of the step


class VitTables(NamedTuple):
    """Packed tables of one transformer flow step (TransCoupling.step_tables)"""
    form: str                # "wave" | "rs": the forward kernel they are laid out for (TransCoupling.step_variant)
    ws: Any                  # forward tables
    winv: Any = None         # Wm^-1 (training, rs)
    wsb: Any = None          # backward kernel's tables (training, rs)


class VStep(NamedTuple):
    """Conv1x1 -> ActNorm -> TransCoupling in one kernel"""
    kind = "vstep"
    conv: Any
    act: Any
    cpl: Any
    x: Any = None
    tables: Any = None       # the forward's VitTables (the backward kernel reads row-split ones: a wave forward's are packed anew)
    xtape: Any = None        # residual-stream tape, or None = recomputed


class Squeeze(NamedTuple):
    kind = "squeeze"
    p: tuple


class Split(NamedTuple):
    """SplitPrior: x is the full tensor before the split"""
    kind = "split"
    dist: Any
    x: Any = None
    prepared: Any = None


class Prior(NamedTuple):
    kind = "prior"
    dist: Any
    x: Any = None
    prepared: Any = None


class Layer(NamedTuple):
    """any other layer, run by its own kernels (autograd_layers.layer_backward)"""
    kind = "layer"
    module: Any
    x: Any = None


# ---- specialist (context-conditioned) flows: each layer's training forward appends its own record, autograd_ctx.SpecialistLogProb
# walks them; besides these the specialist tape holds Pre and Squeeze.  c: the code of the layer's context encoder, eps: the
# Gaussian draw of a flow-type encoder (flowlayer.encoder_noise) or None
class Permute(NamedTuple):
    kind = "permute"
    inverse: tuple           # undoes the map the pass applied: PermuteAxes.inverse_permutation (.permutation on the backward walk)


class CtxAffine(NamedTuple):
    """Conv1x1 / ActNorm with a context net: m = CN(c), the per-sample matrix / shift and log-scale"""
    kind = "ctx_affine"
    module: Any
    x: Any
    c: Any
    m: Any
    eps: Any


class CtxCoupling(NamedTuple):
    """Coupling with a context net, fused step kernel: a1, a2, cn = the activations of its CN chain"""
    kind = "ctx_coupling"
    module: Any
    x: Any
    c: Any
    a1: Any
    a2: Any
    cn: Any
    ws: Any                  # packed forward tables
    mode: int                # 1: CN(c) on the conditioner output (contextflow), 2: in front of its first ReLU
    planes: Any              # step_tape(...) of the forward (mode 2), else None
    eps: Any


class CtxTransCoupling(NamedTuple):
    kind = "ctx_transcoupling"
    module: Any
    x: Any
    c: Any
    a1: Any
    a2: Any
    cn: Any
    eps: Any


class CtxMixture(NamedTuple):
    """context-shifted mixture (a SplitPrior's or the final prior): x is the part it scores, c the embedding rows"""
    kind = "ctx_mixture"
    dist: Any
    x: Any
    c: Any
    logw: Any
    context: Any
    lp: Any                  # per-component log-joints of the forward
    tab: Any                 # (key, inv, dsig, lsum) scale tables of the embedding-lookup form, or None


# ---- the differentiable backward walk (autograd_inverse.walk writes one per inverted group, autograd_inverse.VJP holds the rule of
# each kind).  Besides these the walk writes Squeeze, and Permute with the layer's FORWARD permutation - the inverse of the map the
# walk applied.
class InvStep(NamedTuple):
    """Conv1x1 <- ActNorm <- Coupling inverted by one kernel (cf_flow_step_inv)"""
    kind = "inv_step"
    conv: Any
    act: Any
    cpl: Any
    x: Any                   # the recovered step input


class InvTail(NamedTuple):
    """the pre-processing tail, in front of a Dequantization"""
    kind = "inv_tail"
    y: Any                   # the tail's input in the walk (the logits)
    keep: int                # channels behind the Augment's reverse
    s12: float               # product of the two Normalizations' scales


class InvSplit(NamedTuple):
    """SplitPrior.reverse: a concatenate"""
    kind = "inv_split"
    c: int                   # channels in front of the concatenate
    given: bool              # the upper half was a latent of `decode` (it gets a gradient), not a draw


class InvConv(NamedTuple):
    kind = "inv_conv"
    module: Any


class InvAct(NamedTuple):
    kind = "inv_act"
    module: Any


class InvScale(NamedTuple):
    """Normalization"""
    kind = "inv_scale"
    s: float


class InvAugment(NamedTuple):
    kind = "inv_augment"
    channels: int            # channels in front of Augment.reverse


class InvCoupling(NamedTuple):
    """Coupling / CouplingFC on the layer path"""
    kind = "inv_coupling"
    module: Any
    y: Any                   # the recovered coupling input


class InvVitStep(NamedTuple):
    """Conv1x1 <- ActNorm <- TransCoupling in the one-kernel geometry: inverted by the plain walk's three launches, its
    vector-Jacobian product one kernel (cf_vit_inv_step_bwd_data)"""
    kind = "inv_vstep"
    conv: Any
    act: Any
    cpl: Any
    x: Any                   # the recovered step input


class InvTransCoupling(NamedTuple):
    """TransCoupling on the layer path (any other geometry, fused = False, an uninitialised ActNorm in front)"""
    kind = "inv_transcoupling"
    module: Any
    y: Any                   # the recovered coupling input


class InvCtxAffine(NamedTuple):
    """[Squeeze <-] Conv1x1(c) <- ActNorm(c'), or either layer alone (cf_affine_ctx_inv)"""
    kind = "inv_affine_ctx"
    operands: Any            # conv1x1.affine_ctx_operands: the per-sample matrices and log-scales of the codes the walk formed
    shape: tuple             # of the group's input in the walk
    unsqueeze: bool


class InvCtxCoupling(NamedTuple):
    """Coupling with a context net inverted by one kernel (cf_flow_step_inv_ctx)"""
    kind = "inv_coupling_ctx"
    module: Any
    x: Any                   # the recovered coupling input
    sbias: Any               # per-sample bias CN(c)
    mode: int                # as CtxCoupling.mode
    ws: Any                  # packed forward tables (identity front)


def data_only(rec):
    """A specialist record with only what the data-only walk (autograd_ctx.input_gradient_ctx) reads: no layer input where the
    backward kernel does not need it, no code, CN activations or encoder noise - and of a mode-2 coupling the aux buffer alone
    (its y0 / h1 / h2 planes, operands of the weight gradients, go back to the allocator with this call)."""
    kind = rec.kind
    if kind == "ctx_affine":
        return rec._replace(x=None, c=None, eps=None)
    if kind == "ctx_coupling":
        if rec.mode == 1:
            return rec._replace(c=None, a1=None, a2=None, eps=None)
        return rec._replace(x=None, c=None, a1=None, a2=None, cn=None, ws=None, planes=(None, None, None, rec.planes[3]), eps=None)
    if kind == "ctx_transcoupling":
        return rec._replace(c=None, a1=None, a2=None, eps=None)
    if kind == "ctx_mixture":
        return rec._replace(context=None)
    return rec
