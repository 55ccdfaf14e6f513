"""Invertible 1x1 convolution (reference: contextflow/layers/conv1x1.py:9-77): the shared matrix of the generalist
and the per-sample triangular matrix CN(c) of the specialist mode (conv1x1.py:34-50)."""
import torch
import torch.nn as nn

from . import _derived, _hip, _tape
from .context import cn_linear
from .flowlayer import FlowLayer, encoder_noise


def slogdet_inverse(W, want_inverse):
    """Device-side log|det W| (and W^-1): one tiny fp64 Gauss-Jordan workgroup, no host sync."""
    C = W.shape[0]
    lad = torch.empty(1, device=W.device, dtype=torch.float32)
    inv = torch.empty(C, C, device=W.device, dtype=torch.float32) if want_inverse else None
    _hip.call("cf_slogdet_inverse", _hip.p(W), C, _hip.p(lad), _hip.p(inv), _hip.stream())
    return lad, inv


def conv1x1_apply(x, W, bias=None):
    x, xbs = _hip.bview(x)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // max(B * C, 1) if B else 1
    out = torch.empty((B,) + tuple(x.shape[1:]), device=x.device, dtype=torch.float32)
    _hip.call("cf_conv1x1_fwd", _hip.p(x), _hip.p(W), _hip.p(bias), _hip.p(out), B, C, HW, xbs, C * HW, _hip.stream())
    return out


def affine_ctx_operands(conv=None, act=None, context=None):
    """(m1, Wm, m2, t, logs) of cf_affine_ctx_inv for the layers given (either may be None): each forms its code through cn_linear,
    exactly as its forward does."""
    m1 = Wm = m2 = t = logs = None
    if act is not None:
        if act.contextflow and not act.is_initialized():
            raise RuntimeError("ActNorm.reverse with a context net under contextflow needs an initialised layer (run one forward first)")
        m2 = cn_linear(act, context).m
        if act.contextflow:
            t, logs = _hip.f32(act.NN_t.detach()), _hip.f32(act.NN_logs.detach())
    if conv is not None:
        m1 = cn_linear(conv, context).m
        Wm = _hip.f32(conv.NN.detach()) if conv.contextflow else None
    return m1, Wm, m2, t, logs


def _lds_refusal(call):
    try:
        return call()
    except RuntimeError as e:
        if "(code -2)" in str(e):              # CF_ERR_UNSUPPORTED: the shape needs more LDS than a CU has
            raise NotImplementedError(str(e)) from None
        raise


def affine_ctx_inverse(z, conv=None, act=None, context=None, unsqueeze=False, operands=None):
    """[Squeeze(2,2) <-] Conv1x1(c) <- ActNorm(c') backwards in one cf_affine_ctx_inv launch: x = W_b^-1 (z exp(l_b) + t_b).  conv /
    act: the layers (either may be None: the other one alone); operands: what affine_ctx_operands returned for them, where the
    caller keeps it.  NotImplementedError where the per-sample matrix and the sample do not fit the LDS of a CU."""
    zv, zbs = _hip.bview(z)
    B, C, H, W = zv.shape
    m1, Wm, m2, t, logs = operands if operands is not None else affine_ctx_operands(conv, act, context)
    x = torch.empty((B, C // 4, 2 * H, 2 * W) if unsqueeze else (B, C, H, W), device=zv.device, dtype=torch.float32)
    _lds_refusal(lambda: _hip.call("cf_affine_ctx_inv", _hip.p(zv), _hip.p(m1), _hip.p(Wm), _hip.p(m2), _hip.p(t), _hip.p(logs), _hip.p(x),
                                   B, C, H, W, zbs, int(unsqueeze), _hip.stream()))
    return x


def affine_ctx_inverse_vjp(gx, operands, shape, unsqueezed=False):
    """The vector-Jacobian product of affine_ctx_inverse, one cf_affine_ctx_inv_bwd_data launch: gz = exp(l_b) (W_b^-T gx) in the
    (B, C, H, W) = shape of the z that call was given; unsqueezed: gx has the layout of its unsqueeze=True output."""
    B, C, H, W = shape
    m1, Wm, m2, _, logs = operands
    gx = _hip.f32(gx).contiguous()
    gz = torch.empty(B, C, H, W, device=gx.device, dtype=torch.float32)
    _lds_refusal(lambda: _hip.call("cf_affine_ctx_inv_bwd_data", _hip.p(gx), _hip.p(m1), _hip.p(Wm), _hip.p(m2), _hip.p(logs), _hip.p(gz),
                                   B, C, H, W, int(unsqueezed), _hip.stream()))
    return gz


class Conv1x1(FlowLayer):
    def __init__(self, data_size, context_net=None, contextflow=False):
        super().__init__()
        D, H, W = data_size if len(data_size) == 3 else (data_size[0], 1, 1)
        self.D, self.H, self.W = D, H, W
        self.NN = nn.Parameter(torch.empty(D, D))          # same parameter name as the reference
        nn.init.orthogonal_(self.NN)
        self.context_net = context_net
        self.contextflow = contextflow
        if self.context_net:                               # conv1x1.py:20-26
            self.C = self.context_net.C
            self.CN = nn.Linear(self.C, D * D)
            nn.init.zeros_(self.CN.weight)
            nn.init.zeros_(self.CN.bias)
            if self.contextflow:
                self.NN.requires_grad_(False)

    def logdet_const(self, HW, dev):
        """(1,) tensor: H W log|det NN| of the shared matrix, kept while NN is unchanged (one factorisation per layer and call
        otherwise) - the frozen matrix under contextflow, and the layer's constant along a backward walk that returns log p."""
        return _derived.get(self, "lad", _derived.key((self.NN,), HW, str(dev)),
                            lambda: slogdet_inverse(_hip.f32(self.NN.detach()), False)[0] * float(HW), dev)

    def _forward_ctx(self, x, context, tape=None, pre=None):
        """conv1x1.py:34-50: per-sample triangular matrix from CN(c).  `tape` (training): receives what the backward
        needs - the encoder is stochastic, so its output must be kept, not recomputed.  pre: the code, its log-density and CN(c)
        already formed by the grouped front end (layers/specialist.py::_front_end)."""
        x, xbs = _hip.bview(x)
        B, C, H, W = x.shape
        cn = cn_linear(self, context, pre)
        Wm = _hip.f32(self.NN.detach()) if self.contextflow else None
        z = torch.empty(B, C, H, W, device=x.device, dtype=torch.float32)
        ldj = torch.empty(B, device=x.device, dtype=torch.float32)
        _hip.call("cf_conv1x1_ctx", _hip.p(x), _hip.p(cn.m), _hip.p(Wm), _hip.p(z), _hip.p(ldj), B, C, H * W, xbs, _hip.stream())
        if self.contextflow:
            ldj = ldj + self.logdet_const(H * W, x.device)
        if tape is not None:
            tape.append(_tape.CtxAffine(self, x, cn.c, cn.m, encoder_noise(self.context_net)))
        return z, ldj + cn.logp * float(H * W)

    def forward(self, x, context=None):
        _hip.require_device(x, self.NN)
        if self.context_net:
            return self._forward_ctx(x, context)
        B, _, H, W = x.shape
        Wm = _hip.f32(self.NN.detach())
        z = conv1x1_apply(x, Wm)
        lad, _ = slogdet_inverse(Wm, False)
        return z, (lad * float(H * W)).expand(B)           # conv1x1.py:53

    def reverse(self, z, context=None):
        _hip.require_device(z, self.NN)
        if self.context_net:
            # by specification (the reference's own is marked 'to update'): the inverse of the map z = W_b x the forward applies
            return affine_ctx_inverse(z, conv=self, context=context)
        # W^-1 follows NN's version counter and storage (`sample` inverts every layer's matrix per call otherwise)
        inv = _derived.get(self, "winv", _derived.key((self.NN,), str(z.device)),
                           lambda: slogdet_inverse(_hip.f32(self.NN.detach()), True)[1], z.device)
        return conv1x1_apply(z, inv)                       # conv1x1.py:72

    def logdet(self, input, context=None):
        return self.forward(input, context)[1]


class FC(Conv1x1):
    """Flat variant (conv1x1.py:80-96)."""

    def __init__(self, data_size, context_net=None, contextflow=False):
        super().__init__(data_size, context_net=None, contextflow=False)

    def forward(self, x, context=None):
        out, ldj = super().forward(x.view(-1, self.D, 1, 1), context)
        return out.view(-1, self.D), ldj

    def reverse(self, z, context=None):
        return super().reverse(z.view(-1, self.D, 1, 1), context).view(-1, self.D)

    def logdet(self, x, context=None):
        return super().logdet(x.view(-1, self.D, 1, 1))
