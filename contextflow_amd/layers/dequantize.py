"""Dequantization (reference: contextflow/layers/dequantize.py:8-23)."""
import math
from collections import namedtuple

import torch

from . import _hip
from .augment import Augment
from .flowlayer import PreprocessingFlowLayer
from .normalize import Normalization
from .transforms import LogitTransform


class Dequantization(PreprocessingFlowLayer):
    def __init__(self, dist):
        super().__init__()
        self.dist = dist          # a distribution with support on [0, 1]^d

    def forward(self, input, context=None):
        _hip.require_device(input)
        noise, log_qnoise = self.dist.sample(input.size(0), context=input)
        x, u = _hip.f32(input), _hip.f32(noise)
        out = torch.empty_like(x)
        _hip.call("cf_dequant_fwd", _hip.p(x), _hip.p(u), _hip.p(out), x.numel(), _hip.stream())
        return out, -log_qnoise

    def reverse(self, input, context=None):
        _hip.require_device(input)
        x = _hip.f32(input)
        out = torch.empty_like(x)
        _hip.call("cf_floor", _hip.p(x), _hip.p(out), x.numel(), _hip.stream())
        return out

    def logdet(self, input, context=None):
        raise NotImplementedError


# The pre-processing group of the image flows (model.py:55-58) as `preprocessing_group` finds it.  aug: the module behind the
# LogitTransform when it is an Augment over the channel axis, else None; count: modules of the group, 4 or 5
PreGroup = namedtuple("PreGroup", "deq n1 n2 logit aug count")


def preprocessing_group(mods, i=0):
    """Dequantization -> Normalization x 2 -> LogitTransform [-> Augment over the channels] at mods[i:], as a PreGroup, or None.
    Structure alone: what a caller needs besides - noise distributions, injected noise, offsets, channel counts - it asks of the
    record, and the callers differ in that on purpose."""
    deq, n1, n2, logit, aug = (tuple(mods[i:i + 5]) + (None,) * 5)[:5]
    if not (isinstance(deq, Dequantization) and isinstance(n1, Normalization) and isinstance(n2, Normalization)
            and isinstance(logit, LogitTransform)):
        return None
    aug = aug if isinstance(aug, Augment) and aug.split_dim == 1 else None
    return PreGroup(deq, n1, n2, logit, aug, 4 if aug is None else 5)


def preprocess_rng_fwd(x, group, aug, ld):
    """The group in ONE launch, its noise drawn inside the kernel (Philox, keyed by torch's seed): the dequantisation uniforms and the
    normals of the channels `aug` adds (None: none) never travel through HBM as tensors.  x (B, C, H, W); ld (B,) is ASSIGNED the
    per-sample log-det.  Returns y (B, C + aug_size, H, W) - or None, without a launch and without a draw, where the kernel does not
    apply: noise injected into either layer, or sizes that are no multiple of its vector width."""
    B, C, H, W = x.shape
    N, ca = C * H * W, (aug.aug_size if aug is not None else 0)
    if (group.deq.dist.fixed_noise is not None or (aug is not None and aug.distribution.fixed_noise is not None)
            or N % 4 != 0 or (ca * H * W) % 4 != 0):
        return None
    n1, n2 = group.n1, group.n2
    xin = _hip.f32(x)
    y = torch.empty(B, C + ca, H, W, device=x.device, dtype=torch.float32)
    cst = -N * math.log(n1._s) - N * math.log(n2._s)          # normalize.py:42-49, twice
    key, nonce = _hip.noise_nonce(x.device)                    # one draw from torch's generator per call; the rank is in the key
    _hip.call("cf_preprocess_rng_fwd", _hip.p(xin), _hip.p(y), _hip.p(ld), _hip.p(nonce), key, B, N, ca * H * W,
              (C + ca) * H * W, n1._t, n1._s, n2._t, n2._s, cst, 0, _hip.stream())
    return y
