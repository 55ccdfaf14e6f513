"""Coupling layers: the affine ones (reference: contextflow/layers/coupling.py:14-159) and SplineCoupling.

Coupling      — conditioner = Conv2d 1x1 -> ReLU -> Conv2d kxk (reflect) -> ReLU -> Conv2d 1x1
TransCoupling — conditioner = SimpleViT
SplineCoupling — conditioner as Coupling's, a monotone rational-quadratic spline per element in place of the affine map
The affine ones transform the SECOND channel half given the first: t = h[:, :C/2], log_s = 2 tanh(h[:, C/2:]/2),
z1 = x1*exp(log_s) + t, ldj = sum log_s (coupling.py:52-66).  The nn.Conv2d / nn.Linear objects are
kept purely as parameter containers so that `state_dict` keys equal the reference's; the arithmetic
runs in the HIP kernels."""
import torch
import torch.nn as nn

from . import _derived, _hip, _tape
from .context import cn_chain
from .flowlayer import FlowLayer, encoder_noise

VIT_EVENTS = None        # bench.py: list collecting (start, end, batch) HIP events per fused ViT-coupling launch
from .simple_vit import SimpleViT


def conv2d_reflect(x, conv, relu):
    """x: (B,Cin,H,W) possibly a channel slice; conv: nn.Conv2d holding weight/bias."""
    x, xbs = _hip.bview(x)
    B, Cin, H, W = x.shape
    w = _hip.f32(conv.weight.detach())
    b = _hip.f32(conv.bias.detach()) if conv.bias is not None else None
    Cout, _, kh, kw = w.shape
    ph, pw = conv.padding if isinstance(conv.padding, tuple) else (conv.padding, conv.padding)
    out = torch.empty(B, Cout, H, W, device=x.device, dtype=torch.float32)
    _hip.call("cf_conv2d_reflect", _hip.p(x), _hip.p(w), _hip.p(b), _hip.p(out), B, Cin, Cout, H, W, kh, kw, ph, pw,
              int(relu), xbs, _hip.stream())
    return out


def coupling_apply(x, h, inverse, inverse_ldj=False):
    """inverse_ldj: the inverse map also returns sum log_s, the forward log-det at the point it recovers (None otherwise)."""
    x, h = _hip.f32(x), _hip.f32(h)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // max(B * C, 1) if B else 1
    z = torch.empty_like(x)
    ldj = None if inverse and not inverse_ldj else torch.empty(B, device=x.device, dtype=torch.float32)
    _hip.call("cf_coupling_apply", _hip.p(x), _hip.p(h), _hip.p(z), _hip.p(ldj), B, C, HW, int(inverse), _hip.stream())
    return z, ldj


def conditioner_sources(cpl):
    """The six parameters of a Coupling's conditioner in the packing kernels' order: weight and bias of its 1x1, 3x3 and last 1x1."""
    c1, c2, c3 = cpl.NN[0], cpl.NN[2], cpl.NN[4]
    return c1.weight, c1.bias, c2.weight, c2.bias, c3.weight, c3.bias


def step_sources(conv, act, cpl):
    """The nine parameters a Conv1x1 -> ActNorm -> Coupling step derives its tables from, in the packing kernels' order.  Every
    cache key of such tables and every launch that packs them takes the tuple, or a slice, from here: both name the same tensors."""
    return (conv.NN, act.NN_t, act.NN_logs) + conditioner_sources(cpl)


def identity_front_step_tables(cpl, w1, C, H, W, dev):
    """Packed tables of the fused flow-step kernel for the Coupling `cpl` alone: an identity 1x1 and a zero ActNorm in front of
    its conditioner.  w1: the weight of the conditioner's first 1x1 (its data columns when CN(c) is concatenated to the input)."""
    f, pp = _hip.f32, _hip.p
    eye = torch.eye(C, device=dev, dtype=torch.float32)
    zero = torch.zeros(C, device=dev, dtype=torch.float32)
    ws = torch.empty(_hip.lib().cf_flow_step_ws_bytes(C, H, W), device=dev, dtype=torch.uint8)
    _hip.call("cf_flow_step_prepare", pp(eye), pp(zero), pp(zero), pp(w1), *[pp(f(t.detach())) for t in conditioner_sources(cpl)[1:]],
              pp(ws), C, H, W, _hip.stream())
    return ws


class _AffineCoupling(FlowLayer):
    def net(self, x0):
        raise NotImplementedError

    def forward(self, x, context=None):
        _hip.require_device(x)
        h = self.net(x[:, : x.shape[1] // 2])
        return coupling_apply(x, h, False)

    def reverse(self, z, context=None):
        _hip.require_device(z)
        h = self.net(z[:, : z.shape[1] // 2])
        return coupling_apply(z, h, True)[0]

    def reverse_ldj(self, z):
        """(x, ldj): `reverse` and the forward log-det at x, from the same conditioner pass (context-free layers)."""
        if self.context_net:
            raise NotImplementedError("reverse_ldj: %s with a context net" % type(self).__name__)
        _hip.require_device(z)
        h = self.net(z[:, : z.shape[1] // 2])
        return coupling_apply(z, h, True, inverse_ldj=True)

    def logdet(self, input, context=None):
        return self.forward(input, context)[1]


class Coupling(_AffineCoupling):
    def __init__(self, data_channels, kernel_size=(1, 1), padding=(0, 0), context_net=None, contextflow=False):
        super().__init__()
        D, Hd, O = data_channels // 2, data_channels * 2, data_channels
        self.context_net = context_net                     # registered before NN, as in the reference (key order)
        self.contextflow = contextflow
        concat = bool(context_net) and not contextflow       # coupling.py:33-34: CN(c) concatenated to the net input
        self.NN = nn.Sequential(
            nn.Conv2d(D + O if concat else D, Hd, 1), nn.ReLU(),
            nn.Conv2d(Hd, Hd, kernel_size, padding=padding, padding_mode="reflect"), nn.ReLU(),
            nn.Conv2d(Hd, O, 1))
        if self.context_net:                               # coupling.py:31-37
            if self.contextflow:
                for p in self.NN.parameters():
                    p.requires_grad_(False)
            self.C = self.context_net.C
            self.CN = nn.Sequential(nn.Linear(self.C, Hd), nn.ReLU(), nn.Linear(Hd, Hd), nn.ReLU(), nn.Linear(Hd, O))
        self.fused = True                                  # specialist: one-kernel path when the geometry allows it

    def net(self, x0):
        h = conv2d_reflect(x0, self.NN[0], True)
        h = conv2d_reflect(h, self.NN[2], True)
        return conv2d_reflect(h, self.NN[4], False)

    def _net_ctx(self, x0, context):
        """coupling.py:39-47: h = NN(x0) + CN(c) (contextflow) or NN([x0 ; CN(c) broadcast]) — the broadcast part of the
        first 1x1 convolution is a per-sample bias W[:, D:] CN(c) + b."""
        code = cn_chain(self, context)
        cn, logp_c = code.cn, code.logp                                                            # cn: (B, O)
        x0, xbs = _hip.bview(x0)
        B, D, H, W = x0.shape
        st = _hip.stream()
        if self.contextflow:
            h = self.net(x0)
            _hip.call("cf_add_sample_bias", _hip.p(h), _hip.p(cn), B, h.shape[1], H * W, 0, st)
            return h, logp_c
        c1 = self.NN[0]
        w = _hip.f32(c1.weight.detach())
        Hd = w.shape[0]
        wx = w[:, :D].contiguous()
        wc = w[:, D:, 0, 0].contiguous()
        bias_b = torch.empty(B, Hd, device=x0.device, dtype=torch.float32)       # W[:, D:] cn_b + b
        _hip.call("cf_linear", _hip.p(cn), _hip.p(wc), _hip.p(_hip.f32(c1.bias.detach())), None, _hip.p(bias_b), B,
                  wc.shape[1], Hd, 0, st)
        h1 = torch.empty(B, Hd, H, W, device=x0.device, dtype=torch.float32)
        _hip.call("cf_conv2d_reflect", _hip.p(x0), _hip.p(wx), None, _hip.p(h1), B, D, Hd, H, W, 1, 1, 0, 0, 0, xbs, st)
        _hip.call("cf_add_sample_bias", _hip.p(h1), _hip.p(bias_b), B, Hd, H * W, 1, st)
        h = conv2d_reflect(h1, self.NN[2], True)
        return conv2d_reflect(h, self.NN[4], False), logp_c

    def _ctx_step_operands(self, cn, C, H, W, dev):
        """(mode, sbias, ws) of the fused coupling step under the code's CN(c) = cn (B, O): the per-sample bias - mode 1, cn itself on
        the conditioner output (contextflow); mode 2, W[:, D:] cn before the first ReLU - and the packed tables with an identity
        front, shared by the forward kernel, the inverse kernel and their backward kernels."""
        B, D = cn.shape[0], C // 2
        st, f, pp = _hip.stream(), _hip.f32, _hip.p
        c1, c2, c3 = self.NN[0], self.NN[2], self.NN[4]
        w1 = f(c1.weight.detach())
        if self.contextflow:
            mode, sbias = 1, cn
        else:
            wc = w1[:, D:, 0, 0].contiguous()
            sbias = torch.empty(B, wc.shape[0], device=dev, dtype=torch.float32)
            _hip.call("cf_linear", pp(cn), pp(wc), None, None, pp(sbias), B, wc.shape[1], wc.shape[0], 0, st)
            mode, w1 = 2, w1[:, :D].contiguous()
        # packed tables of the step: kept while the conditioner is unchanged (version counter + storage of its six tensors) - under
        # contextflow it is frozen, and a training step otherwise factorises an identity and packs the same tables for every coupling
        srcs = (c1.weight, c1.bias, c2.weight, c2.bias, c3.weight, c3.bias)
        ws = _derived.get(self, "ctx_ws", _derived.key(srcs, mode, C, H, W, str(dev)),
                          lambda: identity_front_step_tables(self, w1, C, H, W, dev), dev)
        return mode, sbias, ws

    def _ctx_step_bwd_tables(self, mode, C, H, W, dev):
        """Transposed fragments of the step-backward kernel for this coupling (identity 1x1 / ActNorm in front), kept while the three
        weights are unchanged."""
        f, pp = _hip.f32, _hip.p
        c1, c2, c3 = self.NN[0], self.NN[2], self.NN[4]

        def build():
            eye = torch.eye(C, device=dev, dtype=torch.float32)
            zero = torch.zeros(C, device=dev, dtype=torch.float32)
            wsb = torch.empty(_hip.lib().cf_flow_step_bwd_ws_bytes(C, H, W), device=dev, dtype=torch.uint8)
            w1 = f(c1.weight.detach())
            w1x = w1 if mode == 1 else w1[:, :C // 2].contiguous()
            _hip.call("cf_flow_step_bwd_prepare", pp(eye), pp(zero), pp(w1x), pp(f(c2.weight.detach())),
                      pp(f(c3.weight.detach())), pp(wsb), C, H, W, _hip.stream())
            return wsb
        return _derived.get(self, "ctx_wsb", _derived.key((c1.weight, c2.weight, c3.weight), mode, C, H, W, str(dev)), build, dev)

    def _fused_ctx(self, x, context, tape=None, pre=None):
        """The Coupling layer as ONE fp32-MFMA kernel (the fused flow-step kernel with an identity 1x1 / ActNorm in
        front) with the CN(c) term as a per-sample bias: on the conditioner output (contextflow) or before its first
        ReLU (CN(c) concatenated to the conditioner input: W[:, D:] CN(c))."""
        code = cn_chain(self, context, pre)         # pre: formed by the grouped front end (layers/specialist.py)
        cn = code.cn                                                                              # (B, O)
        x, xbs = _hip.bview(x)
        B, C, H, W = x.shape
        dev, st, pp = x.device, _hip.stream(), _hip.p
        mode, sbias, ws = self._ctx_step_operands(cn, C, H, W, dev)
        z = torch.empty(B, C, H, W, device=dev, dtype=torch.float32)
        ldj = torch.zeros(B, device=dev, dtype=torch.float32)
        planes = None
        if tape is not None and mode == 2:
            # every parameter trains: the forward kernel also writes the step tape for the backward kernel and the weight gradients
            planes = _tape.step_tape(B, C, H, W, dev)
            _hip.call("cf_flow_step_fwd_ctx_taped", pp(x), pp(z), pp(ldj), pp(ws), pp(sbias), pp(planes[0]), pp(planes[1]),
                      pp(planes[2]), pp(planes[3]), B, C, H, W, xbs, st)
        else:
            # training under contextflow (tape, mode 1): the backward kernel rebuilds the conditioner in the direct form of the 3x3,
            # so the forward that produces the loss keeps that form too (flag 4) - same ReLU masks on both sides
            _hip.call("cf_flow_step_fwd_ctx", pp(x), pp(z), pp(ldj), pp(ws), pp(sbias), mode | (4 if tape is not None else 0), B, C, H, W,
                      xbs, st)
        if tape is not None:
            tape.append(_tape.CtxCoupling(self, x, code.c, code.a1, code.a2, cn, ws, mode, planes, encoder_noise(self.context_net)))
        return z, ldj + code.logp * float(H * W)

    def _fused_ctx_ok(self, x):
        k = self.NN[2]
        return (self.fused and x.dim() == 4 and tuple(k.kernel_size) == (3, 3) and tuple(k.padding) == (1, 1)
                and bool(_hip.lib().cf_flow_step_supported(x.shape[1], x.shape[2], x.shape[3], 3, 3)))

    def forward(self, x, context=None):
        if not self.context_net:
            return super().forward(x, context)
        _hip.require_device(x)
        return self._forward_ctx(x, context)

    def _forward_ctx(self, x, context, tape=None, pre=None):
        """tape (training): receives the layer's record; pre: the front end's entry for this layer, or None."""
        if self._fused_ctx_ok(x):
            return self._fused_ctx(x, context, tape, pre)
        if tape is not None:
            raise NotImplementedError("specialist training needs the fused coupling geometry (3x3, C in 8..64)")
        h, logp_c = self._net_ctx(x[:, : x.shape[1] // 2], context)
        z, ldj = coupling_apply(x, h, False)
        return z, ldj + logp_c * float(x.shape[2] * x.shape[3])

    def reverse(self, z, context=None):
        if not self.context_net:
            return super().reverse(z, context)
        _hip.require_device(z)
        h, _ = self._net_ctx(z[:, : z.shape[1] // 2], context)
        return coupling_apply(z, h, True)[0]


def spline_coupling_apply(x, h, bins, tail_bound, inverse, inverse_ldj=False):
    """[x0 | RQS(x1; h)] (inverse: RQS^-1) and the forward log-det (cf_spline_coupling).  x may be a batch-strided slice;
    inverse_ldj: the inverse map also returns the forward log-det at the point it recovers (None otherwise)."""
    x, xbs = _hip.bview(x)
    h = _hip.f32(h)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // max(B * C, 1) if B else 1
    z = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    ldj = None if inverse and not inverse_ldj else torch.empty(B, device=x.device, dtype=torch.float32)
    _hip.call("cf_spline_coupling", _hip.p(x), _hip.p(h), _hip.p(z), _hip.p(ldj), B, C, HW, bins, float(tail_bound), xbs,
              int(inverse), _hip.stream())
    return z, ldj


class SplineCoupling(FlowLayer):
    """Rational-quadratic spline coupling: z = [x0 | RQS(x1; NN(x0))], the monotone spline with linear tails of
    `SplineActivation` (layers/splines/rational_quadratic.py:21-176) with the knots of every element read from the
    conditioner output (the layout sketched at layers/activations.py:140): channel c (3 bins - 1) + j of NN(x0) belongs to
    data channel c - `bins` unnormalised widths, `bins` heights, `bins - 1` interior derivatives.  The conditioner has the
    shape and the state-dict keys of `Coupling.NN` with a wider last convolution; that one starts at zero, so a fresh layer
    is the identity on [-tail_bound, tail_bound] (outside it always is).  No context variant."""

    def __init__(self, data_channels, kernel_size=(1, 1), padding=(0, 0), bins=8, tail_bound=3.0):
        super().__init__()
        if data_channels < 2 or data_channels % 2:
            raise ValueError("SplineCoupling: data_channels must be even and positive, got %r" % (data_channels,))
        if not 2 <= bins <= 16:
            raise ValueError("SplineCoupling: bins must be in 2..16, got %r" % (bins,))
        if not tail_bound > 0:
            raise ValueError("SplineCoupling: tail_bound must be positive, got %r" % (tail_bound,))
        D, Hd = data_channels // 2, data_channels * 2
        self.context_net = None
        self.bins, self.tail_bound = int(bins), float(tail_bound)
        self.NN = nn.Sequential(
            nn.Conv2d(D, Hd, 1), nn.ReLU(),
            nn.Conv2d(Hd, Hd, kernel_size, padding=padding, padding_mode="reflect"), nn.ReLU(),
            nn.Conv2d(Hd, D * (3 * self.bins - 1), 1))
        nn.init.zeros_(self.NN[4].weight)
        nn.init.zeros_(self.NN[4].bias)

    net = Coupling.net                      # the same three convolutions over self.NN

    def forward(self, x, context=None):
        _hip.require_device(x)
        return spline_coupling_apply(x, self.net(x[:, : x.shape[1] // 2]), self.bins, self.tail_bound, False)

    def reverse(self, z, context=None):
        _hip.require_device(z)
        return spline_coupling_apply(z, self.net(z[:, : z.shape[1] // 2]), self.bins, self.tail_bound, True)[0]

    def reverse_ldj(self, z):
        """(x, ldj): `reverse` and the forward log-det at x, from the same conditioner pass."""
        _hip.require_device(z)
        return spline_coupling_apply(z, self.net(z[:, : z.shape[1] // 2]), self.bins, self.tail_bound, True, inverse_ldj=True)

    def logdet(self, input, context=None):
        return self.forward(input, context)[1]


class CouplingFC(Coupling):
    def __init__(self, data_channels, kernel_size=(1, 1), padding=(0, 0), context_net=None, contextflow=False):
        super().__init__(data_channels, kernel_size=(1, 1), padding=(0, 0), context_net=None, contextflow=False)
        self.D = data_channels

    def forward(self, x, context=None):
        out, ldj = super().forward(x.view(-1, self.D, 1, 1), context)
        return out.view(-1, self.D), ldj

    def reverse(self, z, context=None):
        return super().reverse(z.view(-1, self.D, 1, 1), context).view(-1, self.D)

    def reverse_ldj(self, z):
        x, ldj = super().reverse_ldj(z.view(-1, self.D, 1, 1))
        return x.view(-1, self.D), ldj

    def logdet(self, x, context=None):
        return super().logdet(x.view(-1, self.D, 1, 1))


class TransCoupling(_AffineCoupling):
    def __init__(self, in_sz, p_sz, context_net=None, contextflow=False):
        super().__init__()
        D, Hd, O = in_sz[0] // 2, in_sz[0] * 2, in_sz[0]
        T = O * p_sz[0] * p_sz[1]                       # transformer width (coupling.py:108)
        self.context_net = context_net
        self.contextflow = contextflow
        self.in_sz, self.p_sz = tuple(in_sz), tuple(p_sz)
        vit = dict(image_size=(in_sz[1], in_sz[2]), patch_size=p_sz, dim=T, depth=6, heads=1, mlp_dim=T)
        self.NN = nn.Sequential(SimpleViT(channels=D, **vit))
        if self.context_net:                               # coupling.py:113-119
            if not self.contextflow:
                self.NN = SimpleViT(channels=D + O, **vit)  # input = [x0 ; CN(c) broadcast]; a direct child (key names)
            else:
                for p in self.NN.parameters():
                    p.requires_grad_(False)
            self.C = self.context_net.C
            self.CN = nn.Sequential(nn.Linear(self.C, Hd), nn.ReLU(), nn.Linear(Hd, Hd), nn.ReLU(), nn.Linear(Hd, O))
        self.fused = True                                # one-kernel path when the geometry allows it

    def net(self, x0):
        """Conditioner output h (layer-by-layer kernels; also the fallback for unsupported geometries)."""
        return self.NN[0](x0)

    def _net_ctx(self, x0, context, pre=None):
        """coupling.py:123-133 with a context net: h = ViT(x0) + CN(c) (contextflow) or ViT([x0 ; CN(c) broadcast]); returns h and
        the code with its CN chain (what a training forward tapes).  Quirk kept: the code's log-density is not multiplied by H*W
        here (unlike Coupling)."""
        code = cn_chain(self, context, pre)
        cn = code.cn                                                                              # (B, O)
        B, _, H, W = x0.shape
        if self.contextflow:
            h = self.NN[0](x0)
            _hip.call("cf_add_sample_bias", _hip.p(h), _hip.p(cn), B, h.shape[1], H * W, 0, _hip.stream())
            return h, code
        xin = torch.cat([_hip.f32(x0), cn.view(B, -1, 1, 1).expand(B, cn.shape[1], H, W)], dim=1)   # concatenation: index op
        return self.NN(xin), code

    # ---- fused path: patchify -> ViT -> un-patchify -> affine map -> log-det in one kernel
    def _fused_ok(self, x):
        if not self.fused or x.dim() != 4:
            return False
        vit = self.NN[0]
        C, H, W = x.shape[1:]
        att = vit.transformer.layers[0][0] if len(vit.transformer.layers) else None
        if att is None or (C, H, W) != self.in_sz:
            return False
        return bool(_hip.lib().cf_vit_supported(C, H, W, self.p_sz[0], self.p_sz[1], vit.dim, att.dim_head, att.heads))

    def step_supported(self, shape):
        """True when Conv1x1 -> ActNorm -> this layer can run as ONE kernel (cf_vit_step_fwd)."""
        if not self.fused or self.context_net or tuple(shape) != self.in_sz:
            return False
        vit = self.NN[0]
        att = vit.transformer.layers[0][0] if len(vit.transformer.layers) else None
        if att is None:
            return False
        C, H, W = shape
        # one predicate for both forms of the forward (the dispatch picks by batch size) and the backward kernel (its depth limit);
        # anything else keeps the layer path
        return bool(_hip.lib().cf_vit_step_supported(C, H, W, self.p_sz[0], self.p_sz[1], vit.dim, att.dim_head, att.heads,
                                                     len(vit.transformer.layers)))

    def step_sources(self):
        """Parameters the packed step workspace derives from (cache key of FlowSequential).  The tuple is built once: walking
        the module tree costs more host time per call than the whole step kernel takes at a batch of 256."""
        entries = self.__dict__.get("_derived")
        src = entries.get("step_src") if entries else None
        if src is None:              # (not a parameter-VALUE entry - no key, no event - but dropped with them: layers/_derived.py)
            src = self.__dict__.setdefault("_derived", {})["step_src"] = tuple(self.NN[0].parameters())
        return src

    # batches up to this size take the row-split form of the step kernel (4 samples per workgroup, an eighth of the serial
    # chain); larger ones the one-wave-per-8-samples form
    STEP_RS_MAX_BATCH = 3584          # measured cross-over (tools/dev/vit_variants.py, round 4, both forms with the fused attention tables): 36 vs 61 us at 2048, 46 vs 61 at 3072, 64 vs 61 at 4096
    STEP_FORMS = {"wave": 0, "rs": 1}         # CF_VIT_FORM_* (include/contextflow_hip.h)

    def step_variant(self, B):
        """'rs' | 'wave': which form of the step kernel a batch of B samples takes (FlowSequential keys its packed
        workspaces on it: the two kernels have their own fragment layouts)."""
        return "rs" if B <= self.STEP_RS_MAX_BATCH else "wave"

    @staticmethod
    def step_tables(items, dev, form, winv=False, bwd=False):
        """Pack Conv1x1 / ActNorm / ViT parameters of SEVERAL steps - items: [(coupling, Wm, t, logs)] - into the fragment order
        of one form of the step kernel (cf_vit_step_prepare_batch; 'rs': one factorisation, one fuse and one packing launch for
        all of them).  winv, bwd ('rs' only): also Wm^-1 / the backward kernel's tables per step.  Returns [_tape.VitTables]."""
        L = _hip.lib()
        cpl0 = items[0][0]
        vit = cpl0.NN[0]
        C, depth, n, fid = cpl0.in_sz[0], len(vit.transformer.layers), len(items), TransCoupling.STEP_FORMS[form]
        if vit.pos_embedding.device != dev:
            vit.pos_embedding = vit.pos_embedding.to(dev).contiguous()
        f, A = _hip.f32, _hip.ptr_array
        byte_bufs = lambda nbytes: [torch.empty(nbytes, device=dev, dtype=torch.uint8) for _ in range(n)]
        ws = byte_bufs(L.cf_vit_step_ws_bytes(C, depth, fid))
        Wm, t, logs = [f(i[1].detach()) for i in items], [f(i[2].detach()) for i in items], [f(i[3].detach()) for i in items]
        flat = [i[0]._flat_params() for i in items]
        wi = [torch.empty(C, C, device=dev, dtype=torch.float32) for _ in range(n)] if winv else [None] * n
        wb = byte_bufs(L.cf_vit_step_bwd_ws_bytes(C, depth)) if bwd else [None] * n
        _hip.call("cf_vit_step_prepare_batch", n, A(Wm), A(t), A(logs), A(flat), _hip.p(_hip.f32(vit.pos_embedding)), A(ws),
                  A(wi) if winv else None, A(wb) if bwd else None, C, depth, fid, _hip.stream())
        return [_tape.VitTables(form, *bufs) for bufs in zip(ws, wi, wb)]

    def step_forward(self, x, tables, ld1, h_out=None, xtape=None):
        """z = TransCoupling(ActNorm(Conv1x1(x))) and ld1 += the step's log-det, one launch of the form `tables` are packed for.
        xtape (training): receives the residual stream at the layer boundaries for cf_vit_step_bwd."""
        x, xbs = _hip.bview(x)
        B, C = x.shape[0], x.shape[1]
        depth = len(self.NN[0].transformer.layers)
        z = torch.empty(B, C, x.shape[2], x.shape[3], device=x.device, dtype=torch.float32)
        with _hip.probe(VIT_EVENTS if xtape is None else None, x.device, B):      # bench.py
            _hip.call("cf_vit_step_fwd", _hip.p(x), _hip.p(z), _hip.p(ld1), _hip.p(tables.ws), _hip.p(h_out), _hip.p(xtape), B, C, depth,
                      xbs, self.STEP_FORMS[tables.form], _hip.stream())
        return z

    def _flat_params(self):
        """The ViT parameters as one flat fp32 tensor in the order the pack kernels read them; kept until a parameter's
        version counter moves (a training step asks for it twice: forward and backward)."""
        src = self.step_sources()
        return _derived.get(self, "flat", _derived.key(src), self._flat_params_build, src[0].device)

    def _flat_params_build(self):
        vit = self.NN[0]
        tpe = vit.to_patch_embedding
        parts = [tpe[1].weight, tpe[1].bias, tpe[2].weight, tpe[2].bias, tpe[3].weight, tpe[3].bias]
        for attn, ff in vit.transformer.layers:
            parts += [attn.norm.weight, attn.norm.bias, attn.to_qkv.weight, attn.to_out.weight,
                      ff.net[0].weight, ff.net[0].bias, ff.net[1].weight, ff.net[1].bias, ff.net[3].weight, ff.net[3].bias]
        parts += [vit.transformer.norm.weight, vit.transformer.norm.bias]
        flat = torch.cat([t.detach().reshape(-1).float() for t in parts])
        # the layout every pack kernel walks (VitFlat, csrc/cf_vit_common.h)
        assert flat.numel() == _hip.lib().cf_vit_flat_params(tpe[1].weight.numel(), vit.dim, len(vit.transformer.layers))
        return flat

    def _fused(self, x, inverse, inverse_ldj=False):
        vit = self.NN[0]
        x, xbs = _hip.bview(x)
        B, C, H, W = x.shape
        p1, p2 = self.p_sz
        pd, dim, depth = (C // 2) * p1 * p2, vit.dim, len(vit.transformer.layers)
        L = _hip.lib()
        flat = self._flat_params()
        st = _hip.stream()
        # the packed table follows the flat parameter tensor (rebuilt when a version counter moves): packed once per parameter version,
        # not once per call (`sample` walks eight such layers per call).  The entry holds `flat`, so its id stays taken.
        def build():
            ws = torch.empty(L.cf_vit_ws_bytes(pd, dim, depth), device=x.device, dtype=torch.uint8)
            _hip.call("cf_vit_prepare", _hip.p(flat), _hip.p(ws), pd, dim, depth, st)
            return flat, ws
        ws = _derived.get(self, "fused_ws", (id(flat), pd, dim, depth, str(x.device)), build, x.device)[1]
        if vit.pos_embedding.device != x.device:
            vit.pos_embedding = vit.pos_embedding.to(x.device).contiguous()
        z = torch.empty(B, C, H, W, device=x.device, dtype=torch.float32)
        ldj = None if inverse and not inverse_ldj else torch.empty(B, device=x.device, dtype=torch.float32)
        with _hip.probe(VIT_EVENTS, x.device, B):                                  # bench.py
            _hip.call("cf_vit_coupling", _hip.p(x), _hip.p(z), _hip.p(ldj), _hip.p(ws), _hip.p(vit.pos_embedding),
                      B, C, H, W, p1, p2, dim, depth, xbs, int(inverse), st)
        return z, ldj

    def forward(self, x, context=None):
        _hip.require_device(x)
        if self.context_net:
            return self._forward_ctx(x, context)
        if self._fused_ok(x):
            return self._fused(x, False)
        return super().forward(x, context)

    def _forward_ctx(self, x, context, tape=None, pre=None):
        h, code = self._net_ctx(x[:, : x.shape[1] // 2], context, pre)
        if tape is not None:
            tape.append(_tape.CtxTransCoupling(self, x, code.c, code.a1, code.a2, code.cn, encoder_noise(self.context_net)))
        z, ldj = coupling_apply(x, h, False)
        return z, ldj + code.logp

    def reverse(self, z, context=None):
        _hip.require_device(z)
        if self.context_net:
            h, _ = self._net_ctx(z[:, : z.shape[1] // 2], context)
            return coupling_apply(z, h, True)[0]
        if self._fused_ok(z):
            return self._fused(z, True)[0]
        return super().reverse(z, context)

    def reverse_ldj(self, z):
        if not self.context_net and self._fused_ok(z):
            _hip.require_device(z)
            return self._fused(z, True, inverse_ldj=True)
        return super().reverse_ldj(z)
