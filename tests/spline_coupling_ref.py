"""SplineCoupling restated in plain torch, in the dtype of its inputs (fp64: the reference of tests/test_spline_coupling.py;
fp32 on the CPU: the rounding floor its bars are built from).  Differentiable: fp64 autograd through it is the reference of
the backward kernel.

The map is the reference's `unconstrained_rational_quadratic_spline(..., tails='linear')` (layers/splines/
rational_quadratic.py:21-176) with per-element parameters: minimum bin width / height / derivative 1e-3, the boundary
derivatives min + softplus(log(exp(1 - min) - 1)) = 1, `searchsorted` with its 1e-6 on the last knot, identity and
log-derivative 0 outside [-tail_bound, tail_bound]."""
import math

import torch
import torch.nn.functional as F

MIN_W = MIN_H = MIN_D = 1e-3
DERIV_CONST = math.log(math.exp(1.0 - MIN_D) - 1.0)


def split_params(h, D, K):
    """Conditioner output (B, D (3K-1), H, W) -> (B, D, H, W, 3K-1): channel c (3K-1) + j belongs to data channel c."""
    B, _, H, W = h.shape
    return h.reshape(B, D, 3 * K - 1, H, W).permute(0, 1, 3, 4, 2)


def _cum(u, mn, tb):
    K = u.shape[-1]
    p = mn + (1.0 - mn * K) * F.softmax(u, dim=-1)
    c = 2.0 * tb * torch.cumsum(p, dim=-1)[..., :-1] - tb
    lo = torch.full_like(u[..., :1], -tb)
    return torch.cat([lo, c, -lo], dim=-1)                       # (..., K+1): -tb, interior knots, +tb


def knots(params, K, tail_bound):
    """params (..., 3K-1) -> cumulative widths (..., K+1), cumulative heights (..., K+1), knot derivatives (..., K+1)."""
    uw, uh, ud = params[..., :K], params[..., K:2 * K], params[..., 2 * K:]
    dv = MIN_D + F.softplus(F.pad(ud, (1, 1)) + DERIV_CONST)
    return _cum(uw, MIN_W, tail_bound), _cum(uh, MIN_H, tail_bound), dv


def bin_index(loc, v):
    """`searchsorted` of the reference: count(v >= knots) - 1 with 1e-6 added to the last knot; clamped like the kernels do."""
    K = loc.shape[-1] - 1
    eps = torch.zeros(K + 1, dtype=loc.dtype)
    eps[-1] = 1e-6
    return ((v[..., None] >= loc + eps).sum(-1) - 1).clamp(0, K - 1)


def rqs(v, params, K, tail_bound, inverse=False):
    """Elementwise map.  v (...), params (..., 3K-1).  Returns (out, lad): forward out = RQS(v), inverse out = RQS^-1(v); lad is
    in both directions the FORWARD log-derivative at the x of the pair (the reference returns its negative for the inverse)."""
    tb = float(tail_bound)
    cw, ch, dv = knots(params, K, tb)
    inside = (v >= -tb) & (v <= tb)
    vc = v.clamp(-tb, tb)
    idx = bin_index(ch if inverse else cw, vc.detach())[..., None]
    g = lambda t, i: t.gather(-1, i)[..., 0]
    w0, h0 = g(cw, idx), g(ch, idx)
    w, h = g(cw, idx + 1) - w0, g(ch, idx + 1) - h0
    d0, d1 = g(dv, idx), g(dv, idx + 1)
    delta = h / w
    s2 = d0 + d1 - 2 * delta
    if inverse:
        u = vc - h0
        a = u * s2 + h * (delta - d0)
        b = h * d0 - u * s2
        c = -delta * u
        th = (2 * c) / (-b - torch.sqrt((b * b - 4 * a * c).clamp_min(0)))
        out = th * w + w0
    else:
        th = (vc - w0) / w
        out = h0 + h * (delta * th * th + d0 * th * (1 - th)) / (delta + s2 * th * (1 - th))
    om = 1 - th
    den = delta + s2 * th * om
    lad = torch.log(delta * delta * (d1 * th * th + 2 * delta * th * om + d0 * om * om)) - 2 * torch.log(den)
    return torch.where(inside, out, v), torch.where(inside, lad, torch.zeros_like(lad))


def coupling_map(x, h, K, tail_bound, inverse=False):
    """The layer map given the conditioner output h = NN(x0) (B, D (3K-1), H, W): ([x0 | RQS^(-1)(x1; h)], ldj (B,)) - ldj the
    forward log-det at the x of the pair in both directions."""
    D = x.shape[1] // 2
    out, lad = rqs(x[:, D:], split_params(h, D, K), K, tail_bound, inverse)
    return torch.cat([x[:, :D], out], dim=1), lad.flatten(1).sum(1)


def conditioner(x0, weights, padding):
    """The conv conditioner: 1x1 -> ReLU -> k x k (reflect padding) -> ReLU -> 1x1.  weights: (w1, b1, w2, b2, w3, b3) in the dtype of x0."""
    w1, b1, w2, b2, w3, b3 = weights
    a = F.relu(F.conv2d(x0, w1, b1))
    ph, pw = padding
    if ph or pw:
        a = F.pad(a, (pw, pw, ph, ph), mode="reflect")
    a = F.relu(F.conv2d(a, w2, b2))
    return F.conv2d(a, w3, b3)


def layer_forward(x, weights, padding, K, tail_bound):
    D = x.shape[1] // 2
    return coupling_map(x, conditioner(x[:, :D], weights, padding), K, tail_bound)
