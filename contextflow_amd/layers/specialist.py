"""Evaluation plan of the specialist (context-conditioned) conv flows: `create_model(generalist=False)`, model.py:117-162.

Layer by layer, a specialist step costs three context encoders, five CN Linears, the per-sample Conv1x1, the per-sample
ActNorm, the coupling step and a dozen tiny bookkeeping kernels (`profiles/r3_spec_fwd_b32768_kstats.txt`).  Here the
layer list is grouped the way `FlowSequential._build_plan` groups the generalist's:

  pre-processing          Dequantization -> Normalization x2 -> LogitTransform [-> Augment]: cf_preprocess_rng_fwd
  [Squeeze ->] Conv1x1(c) -> ActNorm(c')    one pass over the sample: cf_affine_ctx_fwd (Squeeze folded into its reads)
  Coupling(c'')           the fused step kernel with the CN(c'') bias, its packed weights kept while the parameters are
                          unchanged, the log-det accumulated in place
  everything else         the layer's own forward

and the per-sample log-dets accumulate in ONE (B,) buffer inside the kernels instead of a (B, M) add per layer.
Evaluation only (no tape); `FlowSequential.forward` uses it under no_grad and falls back to the layer loop when a
model does not have this shape."""
import torch

from . import _derived, _hip
from .actnorm import ActNorm
from .context import ContextCode, cn_chain, cn_linear
from .conv1x1 import Conv1x1, slogdet_inverse
from .coupling import Coupling, conditioner_sources, identity_front_step_tables
from .dequantize import preprocess_rng_fwd, preprocessing_group
from .distributions.gaussian import StandardNormal
from .distributions.uniform import UniformDistribution
from .squeeze import Squeeze


def _const_logp(net):
    """Host constant of an encoder's log-density, or None when it depends on the sample."""
    return getattr(net, "const_logp", None)


class _Acc:
    """Running log-dets: ld1 (B,) per-sample terms, ldM (B, M) per-mixture terms; kernels accumulate into ld1 in place."""

    def __init__(self, B, dev):
        self.B, self.dev, self.ld1, self.ldM, self.cadd = B, dev, None, None, 0.0

    def add(self, ldj):
        if ldj.dim() == 2:
            self.ldM = ldj if self.ldM is None else self.ldM + ldj
            return
        if ldj.dim() == 0:
            ldj = ldj.reshape(1)
        if self.ld1 is None:         # the first term becomes the buffer the kernels accumulate into: never a view / a broadcast
            self.ld1 = ldj.expand(self.B).clone() if (ldj.shape[0] != self.B or ldj.stride(0) == 0 or ldj._base is not None) else ldj
        else:
            self.ld1 += ldj

    def buffer(self):
        """(ld1 buffer, accumulate flag) for a kernel that assigns or accumulates its per-sample log-det."""
        if self.ld1 is None:
            self.ld1 = torch.empty(self.B, device=self.dev, dtype=torch.float32)
            return self.ld1, 0
        return self.ld1, 1

    def zeroed(self):
        if self.ld1 is None:
            self.ld1 = torch.zeros(self.B, device=self.dev, dtype=torch.float32)
        return self.ld1


def _affine_ok(conv, act, shape):
    return (isinstance(conv, Conv1x1) and isinstance(act, ActNorm) and bool(conv.context_net) and bool(act.context_net)
            and len(shape) == 3 and conv.D == shape[0] and act.D == shape[0] and shape[0] <= 128
            and (not act.contextflow or act.is_initialized()))


def _coupling_ws(flow, cpl, C, H, W, dev):
    """Packed weights of the coupling step (identity 1x1 / ActNorm in front), kept while the conditioner is unchanged."""
    srcs = conditioner_sources(cpl)
    return _derived.get(flow, ("spec_ws", id(cpl)), _derived.key(srcs, C, H, W, str(dev)),
                        lambda: identity_front_step_tables(cpl, _hip.f32(srcs[0].detach()), C, H, W, dev), dev)


def _lad(flow, conv, dev):
    """log|det NN| of a frozen Conv1x1 (device scalar), kept while NN is unchanged."""
    return _derived.get(flow, ("spec_lad", id(conv)), _derived.key((conv.NN,), str(dev)),
                        lambda: slogdet_inverse(_hip.f32(conv.NN.detach()), False)[0], dev)


def blocked_rows(C):
    """Row order of Conv1x1.CN for the blocked form of the per-sample matrix (cf_affine_ctx_fwd, m1_blocked): the 16 x 16
    blocks (rt, g <= rt) on and below the diagonal, row-major inside - entry (16 rt + n, 16 g + c) of the (C, C) matrix."""
    idx = []
    for rt in range(C // 16):
        for g in range(rt + 1):
            for n in range(16):
                idx.extend((16 * rt + n) * C + 16 * g + c for c in range(16))
    return idx


def _cn_blocked(flow, conv, C, dev):
    """Conv1x1.CN with its rows in blocked order (weight (Nc, width), bias (Nc)), kept while the CN parameters are unchanged:
    the blocks above the diagonal of the per-sample matrix are never computed, written or read."""
    w, b = conv.CN.weight, conv.CN.bias

    def build():
        idx = torch.tensor(blocked_rows(C), device=dev, dtype=torch.long)
        return _hip.f32(w.detach())[idx].contiguous(), _hip.f32(b.detach())[idx].contiguous()
    return _derived.get(flow, ("spec_cnb", id(conv)), _derived.key((w, b), str(dev)), build, dev)


def supported(flow):
    """True when the plan below has something to fuse: a specialist model with at least one Conv1x1(c) -> ActNorm(c') pair."""
    mods = flow.sequence_modules
    return any(isinstance(m, Conv1x1) and m.context_net and i + 1 < len(mods) and isinstance(mods[i + 1], ActNorm)
               and mods[i + 1].context_net for i, m in enumerate(mods))


def _draw_encoder_noise(flow, B, dev):
    """One torch.rand for the dequantisation noise of ALL uniform context encoders of the flow (three per step: 36 launches
    of a few microseconds each in the cifar10 flow); every encoder picks up its (B, width) slice at its next call.  The
    stream of torch's generator is consumed in module order, (n, B, width) at once instead of n times (B, width)."""
    from .context import ContextEncoder, UniformCatDequantization
    encs = flow.__dict__.get("_spec_encs")
    if encs is None:
        encs = flow.__dict__["_spec_encs"] = [m[1] for m in flow.modules()
                                              if isinstance(m, ContextEncoder) and isinstance(m[1], UniformCatDequantization)]
    live = [e for e in encs if e.fixed_noise is None]
    if len(live) < 2:
        return
    width = max(e.D for e in live)
    u = torch.rand(len(live), B, width, device=dev, dtype=torch.float32)
    for i, e in enumerate(live):
        e.__dict__["_noise_once"] = u[i] if e.D == width else u[i, :, :e.D].contiguous()


FRONT_END = True      # _front_end (False: the module-by-module walk, the reference path of the tests)


def _uniform_encoder(net):
    """(encoder, card, onehot) when `net` is a ContextEncoder whose code is the uniform dequantisation of the one-hot code / of the
    context itself (the form cf_linear_group can build while it stages its input), else None."""
    from .context import ContextEncoder, EyeEncoder, OneHotEncoder, UniformCatDequantization
    if not isinstance(net, ContextEncoder) or not isinstance(net[1], UniformCatDequantization):
        return None
    if isinstance(net[0], OneHotEncoder):
        return net[1], net[0].cardinalities, 1
    if isinstance(net[0], EyeEncoder):
        return net[1], None, 0
    return None


def _front_end(flow, context, B, dev, train=False):
    """Everything a specialist flow computes from the CONTEXT ALONE, ahead of the data path and in three launches instead of ~96:
    the code of every uniform context encoder is formed inside the first Linear that consumes it (Conv1x1.CN, ActNorm.CN,
    Coupling.CN[0]: one grouped launch, cf_linear_group with ctx), then the second and third Linears of the coupling CN nets
    (one grouped launch each).  Returns {id(layer): ContextCode}: m (and blocked) for Conv1x1, m for ActNorm, a1 / a2 / cn for Coupling.
    train (layers/autograd_ctx.py): the training forward's form - the code c and its log-density logp are kept too (everything the
    backward needs), the per-sample matrix in full (C, C) form, couplings with and without contextflow."""
    import ctypes
    mods, n = flow.sequence_modules, len(flow.sequence_modules)
    if not torch.is_tensor(context) or context.dim() != 2 or not FRONT_END:
        return {}
    f = _hip.f32
    first, second, third, out = [], [], [], {}
    enc0 = None
    for i, m in enumerate(mods):
        net = getattr(m, "context_net", None)
        ue = _uniform_encoder(net) if net else None
        if ue is None:
            continue
        enc, card, onehot = ue
        key = (enc.D, onehot, tuple(net.contexts), context.shape[1])   # the code layout: width, kind, cardinalities of the variables
        if enc0 is None:
            enc0 = (key, enc, card, onehot)
        if isinstance(m, (Conv1x1, ActNorm)):
            first_lin = m.CN
        elif type(m) is Coupling and (m.contextflow or train):
            first_lin = m.CN[0]
        else:
            continue
        if (key != enc0[0] or enc.qbins.device != dev or first_lin.weight.device != dev or context.shape[1] != len(net.contexts)
                or first_lin.weight.shape[1] != enc.D or (not onehot and enc.D != context.shape[1])):
            continue                                       # another code layout / device, or a context of another width: the layer's own path
        u = enc.fixed_noise
        if u is not None and tuple(u.shape) != (B, enc.D):
            continue                                       # (the layer's own path reports it)
        if u is None:
            u = enc.__dict__.pop("_noise_once", None)
            if u is None or u.shape != (B, enc.D):
                u = torch.rand((B, enc.D), device=dev, dtype=torch.float32)
        u = f(u.to(dev))                                   # raw pointers travel in host arrays below: everything on `dev`, fp32, dense
        cbuf, lc = None, None
        if train:
            cbuf = torch.empty(B, enc.D, device=dev, dtype=torch.float32)
            lc = getattr(enc, "_lc", None)
            if lc is None or lc.device != dev:
                lc = enc._lc = (enc.ldj_per_dim * enc.D).sum(-1).reshape(1)             # dequantize.py:62, as UniformCatDequantization.encode
            lc = lc.expand(B)
        if isinstance(m, Conv1x1):
            C = m.D
            nblk = 0 if train else _hip.lib().cf_affine_ctx_blocked_floats(C, m.H, m.W)
            if nblk and nblk < C * C:
                w, b = _cn_blocked(flow, m, C, dev)
                blocked = 1
            else:
                w, b, blocked = f(m.CN.weight.detach()), f(m.CN.bias.detach()), 0
            y = torch.empty(B, w.shape[0], device=dev, dtype=torch.float32)
            first.append((u, enc.qbins, w, b, y, 0, cbuf))
            out[id(m)] = ContextCode(cbuf, lc, m=y, blocked=blocked)
        elif isinstance(m, ActNorm):
            w, b = f(m.CN.weight.detach()), f(m.CN.bias.detach())
            y = torch.empty(B, w.shape[0], device=dev, dtype=torch.float32)
            first.append((u, enc.qbins, w, b, y, 0, cbuf))
            out[id(m)] = ContextCode(cbuf, lc, m=y)
        elif type(m) is Coupling and (m.contextflow or train):
            l0, l1, l2 = m.CN[0], m.CN[2], m.CN[4]
            a1 = torch.empty(B, l0.weight.shape[0], device=dev, dtype=torch.float32)
            a2 = torch.empty(B, l1.weight.shape[0], device=dev, dtype=torch.float32)
            cn = torch.empty(B, l2.weight.shape[0], device=dev, dtype=torch.float32)
            first.append((u, enc.qbins, f(l0.weight.detach()), f(l0.bias.detach()), a1, 2, cbuf))
            second.append((a1, None, f(l1.weight.detach()), f(l1.bias.detach()), a2, 2, None))
            third.append((a2, None, f(l2.weight.detach()), f(l2.bias.detach()), cn, 0, None))
            out[id(m)] = ContextCode(cbuf, lc, a1=a1, a2=a2, cn=cn)
    if not first:
        return {}
    _, enc, card, onehot = enc0
    ctx = context.to(device=dev, dtype=torch.int64).contiguous()
    st = _hip.stream()

    def launch(probs, K, with_ctx):
        # problems of one launch share K; the coupling nets of different levels have different hidden widths: one launch per K
        byk = {}
        for pr in probs:
            byk.setdefault(pr[2].shape[1], []).append(pr)
        for k, ps in byk.items():
            nn_ = len(ps)
            arr = lambda j: (ctypes.c_void_p * nn_)(*[(pr[j].data_ptr() if pr[j] is not None else None) for pr in ps])
            Ns = (ctypes.c_int * nn_)(*[pr[2].shape[0] for pr in ps])
            acts = (ctypes.c_int * nn_)(*[pr[5] for pr in ps])
            _hip.call("cf_linear_group", nn_, arr(0), arr(1), arr(2), arr(3), arr(4), arr(6) if (with_ctx and train) else None, Ns, acts,
                      _hip.p(ctx) if with_ctx else None, _hip.p(card) if (with_ctx and card is not None) else None,
                      ctx.shape[1] if with_ctx else 0, onehot if with_ctx else 0, B, k, st)
    launch(first, enc.D, True)
    launch(second, 0, False)
    launch(third, 0, False)
    return out


def forward_eval(flow, x, context):
    """(z, logp (B, M)) of a specialist flow, evaluation.  Same results as FlowSequential._forward_layers to fp32 rounding
    (the per-sample log-dets are summed in another order)."""
    mods, n = flow.sequence_modules, len(flow.sequence_modules)
    B, dev = x.shape[0], x.device
    _draw_encoder_noise(flow, B, dev)
    pre = _front_end(flow, context, B, dev)
    acc = _Acc(B, dev)
    st, pp, f = _hip.stream(), _hip.p, _hip.f32
    i = 0
    while i < n:
        m = mods[i]
        shape = tuple(x.shape[1:])
        # ---- pre-processing in one kernel, noise drawn inside it (as the generalist's plan does)
        # (FlowSequential._build_plan's conditions; without in-kernel noise - injected noise, odd sizes - the layers run one by one, below)
        g = preprocessing_group(mods, i) if len(shape) == 3 else None
        if g is not None and isinstance(g.deq.dist, UniformDistribution):
            aug = g.aug if g.aug is not None and isinstance(g.aug.distribution, StandardNormal) else None
            ldp = torch.empty(B, device=dev, dtype=torch.float32)
            y = preprocess_rng_fwd(x, g, aug, ldp)
            if y is not None:
                acc.add(ldp)
                x = y
                i += 5 if aug is not None else 4
                continue
        # ---- [Squeeze ->] Conv1x1(c) -> ActNorm(c')
        sq = (isinstance(m, Squeeze) and tuple(m.p) == (2, 2) and len(shape) == 3 and shape[1] % 2 == 0 and shape[2] % 2 == 0)
        j = i + 1 if sq else i
        sshape = (shape[0] * 4, shape[1] // 2, shape[2] // 2) if sq else shape
        if j + 1 < n and _affine_ok(mods[j], mods[j + 1], sshape):
            conv, act = mods[j], mods[j + 1]
            C, H, W = sshape
            xv, xbs = _hip.bview(x)
            aligned = xbs % 4 == 0 and xv.data_ptr() % 16 == 0
            cn1 = pre.get(id(conv))                                # formed by the front end (grouped launch)
            if cn1 is None or (cn1.blocked and not aligned):
                nblk = _hip.lib().cf_affine_ctx_blocked_floats(C, H, W) if aligned else 0
                if nblk and nblk < C * C:                          # (B, 10/16 C*C) at C = 64, 3/4 at C = 32: lower blocks only
                    c1, lp1 = conv.context_net(context)
                    wp, bp = _cn_blocked(flow, conv, C, dev)
                    c1f = f(c1)
                    m1 = torch.empty(B, nblk, device=dev, dtype=torch.float32)
                    _hip.call("cf_linear", pp(c1f), pp(wp), pp(bp), None, pp(m1), B, c1f.shape[1], nblk, 0, st)
                    cn1 = ContextCode(c1f, lp1, m=m1, blocked=1)
                else:
                    cn1 = cn_linear(conv, context)                 # m: (B, C*C)
            cn2 = cn_linear(act, context, pre.get(id(act)))        # m: (B, 2C)
            cadd = 0.0
            for net, code in ((conv.context_net, cn1), (act.context_net, cn2)):
                k = _const_logp(net)
                if k is not None:
                    cadd += k * float(H * W)
                else:
                    acc.add(code.logp * float(H * W))
            Wm = f(conv.NN.detach()) if conv.contextflow else None
            t = f(act.NN_t.detach()) if act.contextflow else None
            logs = f(act.NN_logs.detach()) if act.contextflow else None
            lad = _lad(flow, conv, dev) if conv.contextflow else None
            z = torch.empty(B, C, H, W, device=dev, dtype=torch.float32)
            buf, accum = acc.buffer()
            _hip.call("cf_affine_ctx_fwd", pp(xv), pp(cn1.m), pp(Wm), pp(cn2.m), pp(t), pp(logs), pp(lad), cadd, pp(z), pp(buf), B, C, H, W,
                      xbs, int(sq), accum, cn1.blocked or 0, st)
            x = z
            i = j + 2
            continue
        # ---- Coupling(c''): the fused step kernel, CN bias on the conditioner output (contextflow)
        if (type(m) is Coupling and m.context_net and m.contextflow and len(shape) == 3 and m._fused_ctx_ok(x)):
            C, H, W = shape
            code = cn_chain(m, context, pre.get(id(m)))
            xv, xbs = _hip.bview(x)
            ws = _coupling_ws(flow, m, C, H, W, dev)
            z = torch.empty(B, C, H, W, device=dev, dtype=torch.float32)
            _hip.call("cf_flow_step_fwd_ctx", pp(xv), pp(z), pp(acc.zeroed()), pp(ws), pp(code.cn), 1, B, C, H, W, xbs, st)
            k = _const_logp(m.context_net)
            if k is not None:
                acc.cadd += k * float(H * W)
            else:
                acc.add(code.logp * float(H * W))
            x = z
            i += 1
            continue
        x, ldj = m(x, context)
        acc.add(ldj)
        i += 1
    logp = flow.dist.log_prob(x, context)
    if acc.ldM is not None:
        logp = logp + acc.ldM
    if acc.ld1 is not None:
        logp = logp + (acc.ld1 + acc.cadd if acc.cadd else acc.ld1).unsqueeze(-1)
    elif acc.cadd:
        logp = logp + acc.cadd
    return x, logp
