"""The differentiable backward walk: `FlowSequential.inverse / decode(..., differentiable=True)`.

The walk runs the layers' reverses as the plain walk (layers/inverse.py) does, but returns the CONTINUOUS point - for a flow whose first layer is a
Dequantization the chain stops in front of it - and keeps, per inverted group, what the vector-Jacobian product (VJP) of that
group needs: references to tensors the walk produces anyway (the recovered input of a fused step, the logits of the tail, the
output of a layer-path coupling).  `backward` then walks the groups in forward order.  It is a data-only walk: the gradient with
respect to z and to every half `decode` put back, no parameter gradient.

The records are the NamedTuples of the last section of layers/_tape.py; `vjp` looks the rule of a record up by its `kind` in VJP.
Rules (g: the gradient at the group's output in the backward walk, i.e. at the FORWARD input of the layers), by record:
  InvSplit     SplitPrior (a concatenate here)     slice: the upper half is that latent's gradient
  Squeeze / Permute                                the index map (squeeze_op / permute)
  InvConv      Conv1x1                             g <- W^-T g            (conv1x1_apply with the transposed cached inverse)
  InvAct       ActNorm                             g <- g e^{logs}
  InvScale     Normalization                       g <- g scale
  InvAugment   Augment.reverse                     zeros into the dropped channels
  InvTail      the pre-processing tail             cf_postprocess_inv_bwd, one pass
  InvCoupling  Coupling / CouplingFC (layer path)  with F the forward coupling at the recovered y: J_F^-T g = (g0 - A^T u, u),
                                      u = g1 e^{-s} (cf_coupling_apply in inverse mode on g with the shift half of h zeroed); A^T u is
                                      the first half of the forward coupling's data backward on upstream (0, u) with gld = 0
  InvStep      fused step                          cf_flow_step_inv_bwd_data, one launch
The transformer flows:
  InvVitStep   TransCoupling <- ActNorm <- Conv1x1 in the one-kernel geometry (smap: C = 26 on 8 x 1 windows; no context nets, an
                                      initialised ActNorm, flow.fused): the walk runs the plain walk's three reverses - its value is
                                      the plain inverse's bit for bit - and keeps the recovered step input; backward is
                                      cf_vit_inv_step_bwd_data, one launch
  InvTransCoupling  a context-free TransCoupling anywhere else (msl, smd, atm; fused = False; an uninitialised ActNorm in front):
                                      the InvCoupling rule with transcoupling_backward for A^T u; the Conv1x1 / ActNorm around it keep
                                      InvConv / InvAct
A specialist flow under its context - the codes are formed ONCE, in the walk, and the records keep the tensors the
VJP needs (m1, m2, the coupling's per-sample bias), not the encoders: backward differentiates the map the forward applied,
whatever a stochastic encoder would draw next:
  InvCtxAffine    [Squeeze <-] Conv1x1(c) <- ActNorm(c'):  cf_affine_ctx_inv forward (as the plain walk), cf_affine_ctx_inv_bwd_data backward:
                                      g <- e^{l_b} (W_b^-T g), the un-squeeze folded into its loads; a lone context Conv1x1 /
                                      ActNorm is the same pair of entry points with one side NULL
  InvCtxCoupling  Coupling(c), fused geometry:     cf_flow_step_inv_ctx forward - ONE launch where the plain walk runs six - keeping x, the bias
                                      and its mode; cf_flow_step_inv_bwd_ctx_data backward
No gradient with respect to a parameter, a code or the context is formed.
Anything else raises NotImplementedError naming the layer."""
import torch

from . import _derived, _hip, _tape
from .actnorm import ActNorm
from .augment import Augment
from .context import cn_chain
from .conv1x1 import Conv1x1, affine_ctx_inverse, affine_ctx_inverse_vjp, affine_ctx_operands, conv1x1_apply, slogdet_inverse
from . import coupling as _cpl
from .coupling import Coupling, TransCoupling, coupling_apply, step_sources
from .dequantize import Dequantization
from .inverse import _inverse_step, _inverse_tables, _step_fusable, _tail_fusable
from .normalize import Normalization
from .permute_axes import PermuteAxes
from .splitprior import SplitPrior
from .squeeze import Squeeze, squeeze_op


def _step_vjp_tables(flow, conv, act, cpl, shape, dev):
    """(ws, wsb, wsv) of a fused step: the forward tables `_inverse_step` keeps, the transposed fragments of the backward kernel and
    the fragments of diag(e^{logs}) Wm^-T (cf_flow_step_inv_bwd_prepare, from the Wm^-1 in wsi) - kept while the step's parameters
    are unchanged, as the tables of `_inverse_step`."""
    C, H, W = shape
    ws, wsi = _inverse_tables(flow, conv, act, cpl, shape, dev)
    f, pp = _hip.f32, _hip.p
    srcs = step_sources(conv, act, cpl)

    def build():
        L, st = _hip.lib(), _hip.stream()
        wsb = torch.empty(L.cf_flow_step_bwd_ws_bytes(C, H, W), device=dev, dtype=torch.uint8)
        _hip.call("cf_flow_step_bwd_prepare", *[pp(f(t.detach())) for t in (srcs[0], srcs[2]) + srcs[3::2]], pp(wsb), C, H, W, st)
        wsv = torch.empty(L.cf_flow_step_inv_bwd_ws_bytes(C, H, W), device=dev, dtype=torch.uint8)
        _hip.call("cf_flow_step_inv_bwd_prepare", pp(wsi), pp(f(srcs[2].detach())), pp(wsv), C, H, W, st)
        return wsb, wsv
    wsb, wsv = _derived.get(flow, ("inv_bwd_ws", id(cpl)), _derived.key(srcs, C, H, W, str(dev)), build, dev)
    return ws, wsb, wsv


def _coupling_vjp(m, y, g):
    """J_F^-T g of a context-free Coupling / CouplingFC / TransCoupling at its recovered input y, from existing kernels only."""
    from .autograd_layers import coupling_conv_backward, transcoupling_backward
    backward = transcoupling_backward if isinstance(m, TransCoupling) else coupling_conv_backward
    shape = g.shape
    if y.dim() == 2:
        y, g = y.view(-1, m.D, 1, 1), g.reshape(-1, m.D, 1, 1)
    half = y.shape[1] // 2
    h = m.net(y[:, :half])
    h[:, :half].zero_()                                   # no shift: (g0, (g1 - 0) e^{-s})
    u = coupling_apply(_hip.f32(g).contiguous(), h, True)[0]
    up = u.clone()
    up[:, :half].zero_()
    gld = torch.zeros(y.shape[0], device=y.device, dtype=torch.float32)
    at_u = backward(m, y, up, gld, params=False)[0][:, :half]
    u[:, :half] -= at_u
    return u.view(shape)


def _vit_step_matches(flow, conv, act, cpl, z):
    """The group TransCoupling <- ActNorm <- Conv1x1 that the forward runs as one kernel (FlowSequential._build_plan, "vstep")."""
    return (flow.fused and z.dim() == 4 and isinstance(cpl, TransCoupling) and isinstance(act, ActNorm) and isinstance(conv, Conv1x1)
            and not conv.context_net and not act.context_net and conv.D == z.shape[1] and act.D == z.shape[1]
            and act.is_initialized() and cpl.step_supported(tuple(z.shape[1:])))


def _vit_step_vjp_tables(flow, conv, act, cpl, dev):
    """(ws, wsb, wsv) of a transformer step: the row-split forward tables, the backward kernel's and the fragments of
    diag(e^{logs}) Wm^-T (cf_vit_inv_step_bwd_prepare, from the Wm^-1 of the same packing call) - kept while the step's parameters
    are unchanged."""
    C = cpl.in_sz[0]
    srcs = (conv.NN, act.NN_t, act.NN_logs) + tuple(cpl.step_sources())

    def build():
        t = TransCoupling.step_tables([(cpl, conv.NN, act.NN_t, act.NN_logs)], dev, "rs", winv=True, bwd=True)[0]
        wsv = torch.empty(_hip.lib().cf_vit_inv_step_bwd_ws_bytes(C), device=dev, dtype=torch.uint8)
        _hip.call("cf_vit_inv_step_bwd_prepare", _hip.p(t.winv), _hip.p(_hip.f32(act.NN_logs.detach())), _hip.p(wsv), C, _hip.stream())
        return t.ws, t.wsb, wsv
    return _derived.get(flow, ("inv_vstep_ws", id(cpl)), _derived.key(srcs, C, str(dev)), build, dev)


def _coupling_ctx_inverse(m, z, context):
    """(x, record) of a specialist Coupling in the fused geometry: cf_flow_step_inv_ctx, one launch."""
    cn = cn_chain(m, context).cn
    zv, zbs = _hip.bview(z)
    B, C, H, W = zv.shape
    mode, sbias, ws = m._ctx_step_operands(cn, C, H, W, zv.device)
    x = torch.empty(B, C, H, W, device=zv.device, dtype=torch.float32)
    _hip.call("cf_flow_step_inv_ctx", _hip.p(zv), _hip.p(x), _hip.p(ws), _hip.p(sbias), mode, B, C, H, W, zbs, _hip.stream())
    return x, _tape.InvCtxCoupling(m, x, sbias, mode, ws)


def walk(flow, z, latents, context=None):
    """(x, records): the continuous backward walk from z (latents: `decode`'s halves in forward order, or None - every SplitPrior
    then draws) and one record per inverted group, in walk order.  context: that of a specialist flow (the caller pins the
    encoders' noise); its layers then take the rules of the context kernels."""
    mods = flow.sequence_modules
    latents = None if latents is None else list(latents)
    spec = context is not None
    rec = []
    i = len(mods) - 1
    while i >= 0:
        m = mods[i]
        if i == 0 and isinstance(m, Dequantization):
            break                                         # the continuous point: the tensor floor() would be applied to
        if spec and z.dim() == 4 and isinstance(m, (ActNorm, Conv1x1)) and m.context_net:
            # the groups of inverse._inverse: ActNorm(c') <- Conv1x1(c) with the Squeeze((2,2)) in front, or either layer alone
            act = m if isinstance(m, ActNorm) else None
            conv = m if act is None else None
            n = 1
            if (act is not None and i >= 1 and isinstance(mods[i - 1], Conv1x1) and mods[i - 1].context_net
                    and mods[i - 1].D == z.shape[1]):
                conv, n = mods[i - 1], 2
            sq = (n == 2 and i >= 2 and isinstance(mods[i - 2], Squeeze) and tuple(mods[i - 2].p) == (2, 2)
                  and z.shape[1] % 4 == 0)
            ops = affine_ctx_operands(conv, act, context)
            shape = tuple(z.shape)
            z = affine_ctx_inverse(z, operands=ops, unsqueeze=sq)
            rec.append(_tape.InvCtxAffine(ops, shape, sq))
            i -= n + int(sq)
            continue
        if spec and type(m) is Coupling and m.context_net and m._fused_ctx_ok(z):
            z, r = _coupling_ctx_inverse(m, z, context)
            rec.append(r)
            i -= 1
            continue
        if not spec and _step_fusable(flow, i, z):
            z = _inverse_step(flow, z, mods[i - 2], mods[i - 1], m)      # the Squeeze in front, if any, runs as its own launch
            rec.append(_tape.InvStep(mods[i - 2], mods[i - 1], m, z))
            i -= 3
            continue
        if not spec and i >= 2 and _vit_step_matches(flow, mods[i - 2], mods[i - 1], m, z):
            z = mods[i - 2].reverse(mods[i - 1].reverse(m.reverse(z)))       # the plain walk's three launches: its values bit for bit
            rec.append(_tape.InvVitStep(mods[i - 2], mods[i - 1], m, z))
            i -= 3
            continue
        if _tail_fusable(flow, i, z):
            y, n1, n2 = z, mods[1], mods[2]
            keep = y.shape[1] - (mods[4].aug_size if i == 4 else 0)
            z = n1.reverse(n2.reverse(mods[3].reverse(y[:, :keep])))
            rec.append(_tape.InvTail(y, keep, n1._s * n2._s))
            break
        if isinstance(m, SplitPrior):
            c = z.shape[1]
            if latents is not None:
                if not latents:
                    raise ValueError("decode: no latent left for the SplitPrior at layer %d" % i)
                z = m.reverse(z, context, latent=latents.pop())
            else:
                z = m.reverse(z, context)
            rec.append(_tape.InvSplit(c, latents is not None))
        elif isinstance(m, Squeeze):
            z = m.reverse(z)
            rec.append(_tape.Squeeze(tuple(m.p)))
        elif isinstance(m, PermuteAxes):
            z = m.reverse(z)
            rec.append(_tape.Permute(m.permutation))
        elif isinstance(m, Conv1x1) and not m.context_net:
            z = m.reverse(z)
            rec.append(_tape.InvConv(m))
        elif isinstance(m, ActNorm) and not m.context_net:
            z = m.reverse(z)
            rec.append(_tape.InvAct(m))
        elif isinstance(m, Normalization):
            z = m.reverse(z)
            rec.append(_tape.InvScale(m._s))
        elif isinstance(m, Augment) and m.split_dim == 1:
            rec.append(_tape.InvAugment(z.shape[1]))
            z = m.reverse(z)
        elif type(m) in (Coupling, _cpl.CouplingFC) and not m.context_net:
            z = m.reverse(z)
            rec.append(_tape.InvCoupling(m, z))
        elif isinstance(m, TransCoupling) and not m.context_net and z.dim() == 4:
            z = m.reverse(z)
            rec.append(_tape.InvTransCoupling(m, z))
        else:
            raise NotImplementedError("differentiable inverse: no vector-Jacobian rule for the reverse of %s%s (layer %d)"
                                      % (type(m).__name__, " with a context net" if getattr(m, "context_net", None) else "", i))
        i -= 1
    return z, rec


def _kernel_vjp(name, x, g, mid, rest):
    """One data-only backward kernel: g made contiguous, gz allocated like x, the call name(x, g, *mid, gz, *rest, stream)."""
    g = g.contiguous()
    gz = torch.empty(x.shape, device=g.device, dtype=torch.float32)
    _hip.call(name, _hip.p(x), _hip.p(g), *mid, _hip.p(gz), *rest, _hip.stream())
    return gz


def _tail_vjp(flow, r, g, halves):
    yv, ybs = _hip.bview(r.y)
    B, C, H, W = yv.shape
    return _kernel_vjp("cf_postprocess_inv_bwd", yv, g, (), (B, r.keep * H * W, (C - r.keep) * H * W, ybs, C * H * W, r.s12))


def _step_vjp(flow, r, g, halves):
    xv, xbs = _hip.bview(r.x)
    B, C, H, W = xv.shape
    tables = _step_vjp_tables(flow, r.conv, r.act, r.cpl, (C, H, W), xv.device)
    return _kernel_vjp("cf_flow_step_inv_bwd_data", xv, g, [_hip.p(t) for t in tables], (B, C, H, W, xbs))


def _vit_step_vjp(flow, r, g, halves):
    xv, xbs = _hip.bview(r.x)
    B, C = xv.shape[0], xv.shape[1]
    tables = _vit_step_vjp_tables(flow, r.conv, r.act, r.cpl, xv.device)
    return _kernel_vjp("cf_vit_inv_step_bwd_data", xv, g, [_hip.p(t) for t in tables],
                       (B, C, len(r.cpl.NN[0].transformer.layers), xbs))


def _coupling_ctx_vjp(flow, r, g, halves):
    B, C, H, W = r.x.shape
    wsb = r.module._ctx_step_bwd_tables(r.mode, C, H, W, r.x.device)
    return _kernel_vjp("cf_flow_step_inv_bwd_ctx_data", r.x, g, (_hip.p(r.ws), _hip.p(wsb), _hip.p(r.sbias), r.mode), (B, C, H, W, C * H * W))


def _split_vjp(flow, r, g, halves):
    if r.given:
        halves.append(g[:, r.c:].contiguous())
    return g[:, :r.c]


def _conv_vjp(flow, r, g, halves):
    m = r.module
    inv = _derived.get(m, "winv", _derived.key((m.NN,), str(g.device)),
                       lambda: slogdet_inverse(_hip.f32(m.NN.detach()), True)[1], g.device)
    shape = g.shape
    if g.dim() == 2:
        g = g.reshape(-1, m.D, 1, 1)
    return conv1x1_apply(g, inv.t().contiguous()).view(shape)


def _act_vjp(flow, r, g, halves):
    logs = _hip.f32(r.module.NN_logs.detach())
    return g * torch.exp(logs).view([1, -1] + [1] * (g.dim() - 2))


def _augment_vjp(flow, r, g, halves):
    full = g.new_zeros((g.shape[0], r.channels) + tuple(g.shape[2:]))
    full[:, : g.shape[1]] = g
    return full


# The rule of each kind `walk` appends: (flow, record, g at the group's output in the walk, halves) -> g at its input; the rule of
# a half `decode` put back appends that half's gradient to `halves`
VJP = {
    "inv_tail": _tail_vjp,
    "inv_step": _step_vjp,
    "inv_split": _split_vjp,
    "squeeze": lambda flow, r, g, halves: squeeze_op(g, r.p, False),
    "permute": lambda flow, r, g, halves: g.permute(r.inverse).contiguous(),
    "inv_conv": _conv_vjp,
    "inv_act": _act_vjp,
    "inv_scale": lambda flow, r, g, halves: g * r.s,
    "inv_augment": _augment_vjp,
    "inv_coupling": lambda flow, r, g, halves: _coupling_vjp(r.module, r.y, g),
    "inv_vstep": _vit_step_vjp,
    "inv_transcoupling": lambda flow, r, g, halves: _coupling_vjp(r.module, r.y, g),
    "inv_affine_ctx": lambda flow, r, g, halves: affine_ctx_inverse_vjp(g, r.operands, r.shape, r.unsqueeze),
    "inv_coupling_ctx": _coupling_ctx_vjp,
}


def vjp(flow, rec, g):
    """(gz, [gradient of every half put back, in forward order]) from g = dL/dx, walking the groups in forward order."""
    halves = []
    g = _hip.f32(g)
    for r in reversed(rec):
        g = VJP[r.kind](flow, r, g, halves)
    return g.contiguous(), halves


class InverseWalk(torch.autograd.Function):
    """x = the continuous backward walk of (z, *halves); backward: the data-only VJP above.  Once differentiable."""

    @staticmethod
    def forward(ctx, flow, n_halves, context, z, *halves):
        with torch.no_grad():
            x, rec = walk(flow, z, list(halves) if n_halves is not None else None, context)
        ctx.flow, ctx.rec, ctx.n = flow, rec, len(halves)
        ctx.spec = context is not None
        if ctx.spec:                     # autograd's own guard: a second backward without retain_graph raises, as for any graph
            ctx.save_for_backward(z)
        ctx.shapes = [tuple(z.shape)] + [tuple(h.shape) for h in halves]
        return x.clone() if x.data_ptr() == z.data_ptr() else x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gx):
        if ctx.spec:
            ctx.saved_tensors
        gz, gh = vjp(ctx.flow, ctx.rec, gx)
        assert len(gh) == ctx.n and tuple(gz.shape) == ctx.shapes[0]
        out = [gz.view(ctx.shapes[0])] + [h.view(s) for h, s in zip(gh, ctx.shapes[1:])]
        need = ctx.needs_input_grad[3:]
        return (None, None, None) + tuple(o if n else None for o, n in zip(out, need))


def run(flow, z, latents, context=None):
    """The differentiable walk: with grad mode on and a latent that requires a gradient the result carries a grad_fn; otherwise
    the same continuous result, detached.  context: a specialist flow's, the caller holds the encoders' noise pinned."""
    _hip.require_device(z)
    halves = [] if latents is None else list(latents)
    if torch.is_grad_enabled() and any(t.requires_grad for t in [z] + halves):
        return InverseWalk.apply(flow, None if latents is None else len(halves), context, z, *halves)
    with torch.no_grad():
        return walk(flow, z.detach(), None if latents is None else [h.detach() for h in halves], context)[0]
