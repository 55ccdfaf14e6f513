"""The plain backward walk of a FlowSequential - what `inverse`, `sample` and `decode` run - as functions of the flow.  The
differentiable walk (layers/autograd_inverse.py) takes its group predicates and its step launch from here; the two stay two
functions: they differ in what they fold into a launch and in the rounding they guarantee."""
import math

import torch

from . import _derived, _hip
from .actnorm import ActNorm
from .augment import Augment
from .conv1x1 import Conv1x1, affine_ctx_inverse
from .coupling import Coupling, CouplingFC, SplineCoupling, TransCoupling, step_sources
from .dequantize import Dequantization, preprocessing_group
from .distributions.gaussian import GaussianMixtureDistribution, StandardNormal, gmm_logprob, gmm_levels_ok, gmm_logprob_levels, GMM_LEVELS_MAX_BATCH
from .distributions.uniform import UniformDistribution
from .normalize import Normalization
from .permute_axes import PermuteAxes
from .splitprior import SplitPrior
from .squeeze import Squeeze
from .transforms import LogitTransform


class _WalkDensity:
    """What a backward walk gathers for the log-density of the point it produces (_inverse, return_logp):
    ld1 (B,) - the forward log-det of every inverted layer at its recovered input and -log q of the channels an Augment drops,
    added by the inverse kernels themselves - and the tensors the priors score, in place: the final z and every split-off half.
    finish(): log p (B, M) = the mixtures' log-densities + ld1, through the kernels the forward uses."""

    def __init__(self, z):
        self.B, self.dev = z.shape[0], z.device
        self.ld1 = torch.zeros(self.B, device=z.device, dtype=torch.float32)
        self.levels = []              # (tensor, prepared mixture tables) in walk order: the prior first
        self.terms = []               # (B, M) log-densities of priors that are no mixtures

    def score(self, dist, x):
        if isinstance(dist, GaussianMixtureDistribution) and not dist.context_net:
            srcs = (dist.mG, dist.sG, dist.wG)
            self.levels.append((x, _derived.get(dist, "walk_prep", _derived.key(srcs, str(self.dev)), dist.prepared, self.dev)))
        elif callable(getattr(dist, "log_prob", None)) and not getattr(dist, "context_net", None):
            lp = dist.log_prob(x)
            self.terms.append(lp.reshape(self.B, -1))
        else:
            raise NotImplementedError("return_logp: no log-density rule for the prior %s" % type(dist).__name__)

    def finish(self, M):
        B, dev = self.B, self.dev
        levels = self.levels[::-1]    # forward order: the halves, then the prior
        ldM = None
        for t in self.terms:
            if t.shape[1] == 1:
                self.ld1 += t[:, 0]
            else:
                ldM = t.clone() if ldM is None else ldM + t
        if not levels:
            return self.ld1.unsqueeze(-1).expand(B, M).clone() if ldM is None else ldM + self.ld1.unsqueeze(-1)
        if B <= GMM_LEVELS_MAX_BATCH and gmm_levels_ok(levels):
            return gmm_logprob_levels(levels, ldM, self.ld1)
        acc = ldM is not None
        if not acc:
            ldM = torch.empty(B, M, device=dev, dtype=torch.float32)
        for x, prep in levels:
            gmm_logprob(x, prep, out=ldM, accumulate=acc)
            acc = True
        logp = torch.empty(B, M, device=dev, dtype=torch.float32)
        _hip.call("cf_logdet_combine", _hip.p(ldM), _hip.p(self.ld1), _hip.p(logp), B, M, _hip.stream())
        return logp


def _inverse_tables(flow, conv, act, cpl, shape, dev):
    """(ws, wsi) of a fused step for the inverse kernel."""
    C, H, W = shape
    # the packed tables of the step (forward fragments of the conditioner, W^-1 and the inverse ActNorm) are kept while the
    # parameters they derive from are unchanged - version counter and storage of every source tensor, as the forward's tables
    # (two factorisations + two packing launches per step and call before: 13 - 17 % of a `sample` call at 16 384 samples)
    srcs = step_sources(conv, act, cpl)

    def build():
        ws = flow._prepare_steps([(conv, act, cpl)], (C, H, W), dev)[0]
        wsi = torch.empty(_hip.lib().cf_flow_step_inv_ws_bytes(C, H, W), device=dev, dtype=torch.uint8)
        _hip.call("cf_flow_step_inv_prepare", *[_hip.p(_hip.f32(t.detach())) for t in srcs[:3]], _hip.p(wsi), C, H, W, _hip.stream())
        return ws, wsi
    return _derived.get(flow, ("inv_ws", id(cpl)), _derived.key(srcs, C, H, W, str(dev)), build, dev)


def _step_fusable(flow, i, z):
    """mods[i - 2 : i + 1] is a Conv1x1 -> ActNorm -> Coupling group that _inverse_step takes at the shape of z."""
    mods = flow.sequence_modules
    return (flow.fused and i >= 2 and z.dim() == 4 and isinstance(mods[i - 1], ActNorm) and mods[i - 1].is_initialized()
            and flow._step_supported(mods[i - 2], mods[i - 1], mods[i], tuple(z.shape[1:])))


def _inverse_step(flow, z, conv, act, cpl, unsqueeze=False, ld=None):
    """Conv1x1^-1 o ActNorm^-1 o Coupling^-1 in one MFMA kernel (cf_flow_step_inv); unsqueeze: the Squeeze((2,2)) in front of
    the step is inverted by the kernel's stores.  ld (B,): the step's forward log-det at the recovered input is added to it
    (cf_flow_step_inv_ld: the same kernel, the same x).  flow.inv_events: a record per launch (bench.py)."""
    z, zbs = _hip.bview(z)
    B, C, H, W = z.shape
    dev = z.device
    pp, st = _hip.p, _hip.stream()
    ws, wsi = _inverse_tables(flow, conv, act, cpl, (C, H, W), dev)
    x = torch.empty((B, C // 4, 2 * H, 2 * W) if unsqueeze else (B, C, H, W), device=dev, dtype=torch.float32)
    with _hip.probe(flow.inv_events, dev, B, C, H * W):
        if ld is None:
            _hip.call("cf_flow_step_inv", pp(z), pp(x), pp(ws), pp(wsi), B, C, H, W, zbs, int(unsqueeze), st)
        else:
            _hip.call("cf_flow_step_inv_ld", pp(z), pp(x), pp(ld), pp(ws), pp(wsi), B, C, H, W, zbs, int(unsqueeze), st)
    return x


def _pixel_range(flow):
    """(0, bins - 1) of the image flows - their pre-processing group with Normalization(0, bins) behind the Dequantization
    (model.py:97-98) - else None.  Asks for the offset _t == 0 and nothing about the noise: the range is a property of the data."""
    g = preprocessing_group(flow.sequence_modules)
    if g is not None and g.n1._t == 0.0:
        return 0.0, g.n1._s - 1.0
    return None


def _reverse_scored(m, z, wd):
    """m.reverse(z) for a layer other than a SplitPrior, with the layer's forward log-det at the recovered input added to the
    walk's running term wd.ld1.  NotImplementedError, naming the layer, where there is no rule."""
    if isinstance(m, (Squeeze, PermuteAxes)):
        return m.reverse(z)                                     # index maps: 0
    if isinstance(m, Conv1x1) and not m.context_net:
        wd.ld1 += m.logdet_const(z.shape[2] * z.shape[3] if z.dim() == 4 else 1, z.device)
        return m.reverse(z)
    if isinstance(m, ActNorm) and not m.context_net:
        wd.ld1 += _hip.f32(m.NN_logs.detach()).sum()            # actnorm.py:58: + sum logs, without the H W factor (the quirk kept)
        return m.reverse(z)
    if type(m) in (Coupling, CouplingFC, TransCoupling, SplineCoupling) and not m.context_net:
        x, ldj = m.reverse_ldj(z)
        wd.ld1 += ldj
        return x
    if isinstance(m, Augment) and m.split_dim == 1 and isinstance(m.distribution, StandardNormal):
        keep = z.shape[1] - m.aug_size
        wd.ld1 -= m.distribution.log_prob(z[:, keep:]).squeeze(-1)          # -log N(e) of the dropped channels, read by stride
        return m.reverse(z)
    if isinstance(m, Dequantization) and isinstance(m.dist, UniformDistribution):
        return m.reverse(z)                                     # uniform noise on [0, 1): log q = 0
    if isinstance(m, Normalization):
        wd.ld1 += m.logdet(z)
        return m.reverse(z)
    if isinstance(m, LogitTransform):
        x = m.reverse(z)
        wd.ld1 += m.logdet(x)                                   # -log v - log(1 - v) at v = sigmoid(z)
        return x
    raise NotImplementedError("return_logp: no log-det rule for the reverse of %s" % type(m).__name__)


def _inverse(flow, z, context, clamp, latents=None, labels=None, temperature=1.0, ctx_draw=False, return_logp=False):
    """`FlowSequential.inverse`; clamp = (lo, hi): the output of the leading Dequantization's reverse is projected into that range.
    return_logp: (x, logp) - the walk also gathers the (B, M) log-density `forward` returns at the continuous point it
    passes through (_WalkDensity); x and the random numbers drawn are those of the plain walk.
    latents: the split-off halves in forward order, put back by the SplitPriors instead of fresh draws (`decode`);
    labels / temperature: passed to every SplitPrior's draw (`sample`).  All at their defaults: the plain chain.
    A specialist flow (context nets, a context given): every ActNorm(c) <- Conv1x1(c) pair - with the Squeeze((2,2)) in front of
    it - is one cf_affine_ctx_inv launch, everything else its own reverse(z, context); ctx_draw: the SplitPriors draw from the
    context-shifted mixtures (`sample` under a context)."""
    if latents is not None:
        latents = list(latents)
    _hip.require_device(z)
    mods = flow.sequence_modules
    i = len(mods) - 1
    spec = context is not None and flow._has_context_nets()
    wd = None
    if return_logp:                      # (the public callers have refused it for a specialist flow)
        with torch.no_grad():
            wd = _WalkDensity(z)
            wd.score(flow.dist, z)
    ld = None if wd is None else wd.ld1
    with torch.no_grad():
        while i >= 0:
            m = mods[i]
            if (spec and isinstance(m, ActNorm) and m.context_net and i >= 1 and z.dim() == 4 and isinstance(mods[i - 1], Conv1x1)
                    and mods[i - 1].context_net and mods[i - 1].D == z.shape[1]):
                sq = i >= 2 and isinstance(mods[i - 2], Squeeze) and tuple(mods[i - 2].p) == (2, 2) and z.shape[1] % 4 == 0
                z = affine_ctx_inverse(z, conv=mods[i - 1], act=m, context=context, unsqueeze=sq)
                i -= 3 if sq else 2
            elif not spec and _step_fusable(flow, i, z):
                sq = i >= 3 and isinstance(mods[i - 3], Squeeze) and tuple(mods[i - 3].p) == (2, 2)
                z = _inverse_step(flow, z, mods[i - 2], mods[i - 1], m, unsqueeze=sq, ld=ld)
                i -= 4 if sq else 3
            elif flow.fused and _tail_fusable(flow, i, z):
                z = _inverse_tail(flow, z, i, clamp, ld=ld)
                i = -1
            else:
                if wd is not None and not isinstance(m, SplitPrior):
                    z = _reverse_scored(m, z, wd)
                elif isinstance(m, SplitPrior) and latents is not None:
                    if not latents:
                        raise ValueError("decode: no latent left for the SplitPrior at layer %d" % i)
                    z = m.reverse(z, context, latent=latents.pop())
                elif isinstance(m, SplitPrior) and ctx_draw:
                    z = m.reverse(z, context, labels=labels, temperature=temperature, ctx_draw=True)
                elif isinstance(m, SplitPrior) and (labels is not None or temperature != 1.0):
                    z = m.reverse(z, context, labels=labels, temperature=temperature)
                else:
                    z = m.reverse(z, context)
                if wd is not None and isinstance(m, SplitPrior):
                    wd.score(m.dist, z[:, z.shape[1] // 2:])     # the half just put back - drawn, or `decode`'s - scored in place
                if i == 0 and clamp is not None and isinstance(m, Dequantization):
                    _hip.call("cf_clamp", _hip.p(z), _hip.p(z), z.numel(), clamp[0], clamp[1], _hip.stream())
                i -= 1
        if wd is not None:
            return z, wd.finish(flow.mixtures)
    return z


def _tail_fusable(flow, i, z):
    """mods[:i + 1] is the pre-processing group of the image flows, whose reverse chain cf_postprocess_inv runs in one pass.
    The reverse draws nothing, so nothing is asked about the noise distributions; it asks for the position (the walk stands on the
    group's last module: i = 3, or 4 on the Augment) and that the Augment leaves channels behind it."""
    g = preprocessing_group(flow.sequence_modules) if z.dim() == 4 and i in (3, 4) else None
    return g is not None and (i == 3 or (g.aug is not None and 0 < g.aug.aug_size < z.shape[1]))


def _inverse_tail(flow, z, i, clamp=None, ld=None):
    """ld (B,): the pre-processing's forward log-det at the continuous point behind z - and -log q of the Augment channels that
    are dropped - is added to it (cf_postprocess_inv_ld: one pass, the same x)."""
    mods = flow.sequence_modules
    z, zbs = _hip.bview(z)
    B, C, H, W = z.shape
    keep = C - (mods[4].aug_size if i == 4 else 0)
    x = torch.empty(B, keep, H, W, device=z.device, dtype=torch.float32)
    n1, n2 = mods[1], mods[2]
    if ld is not None:
        N = keep * H * W
        cst = -N * math.log(n1._s) - N * math.log(n2._s)          # normalize.py:42-49, twice (as the forward's `pre`)
        lo, hi = clamp if clamp is not None else (0.0, 0.0)
        _hip.call("cf_postprocess_inv_ld", _hip.p(z), _hip.p(x), _hip.p(ld), B, N, (C - keep) * H * W, zbs, n2._t, n2._s, n1._t, n1._s,
                  cst, int(clamp is not None), lo, hi, _hip.stream())
    elif clamp is None:
        _hip.call("cf_postprocess_inv", _hip.p(z), _hip.p(x), B, keep * H * W, zbs, n2._t, n2._s, n1._t, n1._s, _hip.stream())
    else:
        _hip.call("cf_postprocess_inv_clamped", _hip.p(z), _hip.p(x), B, keep * H * W, zbs, n2._t, n2._s, n1._t, n1._s,
                  clamp[0], clamp[1], _hip.stream())
    return x
