"""Plain torch references of the specialist training backward (tests/test_specialist_backward_fp64.py): the context-shifted
mixture prior, the per-sample Conv1x1 and ActNorm, in any dtype.  No project import except the oracle, which the test ties
these restatements to; everything here runs on the CPU.

Three kinds of reference for the mixture:
  * mixture_autograd     torch.autograd through mixture_logjoints (the formula of oracle.flow_oracle.gmm_ctx_logprob with the
                         shifts c as leaves instead of embedding rows);
  * mixture_given_lp     the closed form of the gradients GIVEN the log-joints lp: r = g softmax_k(lp) and sums of r-weighted
                         terms.  With the kernel's own lp cast to double it holds the arithmetic behind the responsibilities
                         to ~1e-7, where the responsibilities themselves carry one ulp of a log-joint of size 1e3 .. 1e4;
  * mixture_param_grads  the same summands given r, summed over the batch (cf_gmm_ctx_pgrad_tab).
`defect` arguments restate, in the reference's own precision, what a wrong kernel would compute (the tests show that each
breaks the bars)."""
import math
import types

import torch
import torch.nn.functional as F

LOG_2PI = math.log(2.0 * math.pi)
GRAD_CAP, GRAD_MIN, FLOOR_FACTOR = 1e-4, 2e-6, 4.0          # the step tests' rule (tests/step_fp64_ref.py)


def rel_err(got, ref):
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.detach().double()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3)


def bar(floor):
    """Closed forms and well-conditioned graphs: min(1e-4, max(2e-6, 4 x floor))."""
    return min(GRAD_CAP, max(GRAD_MIN, FLOOR_FACTOR * floor))


def bar_mixture(floor):
    """Mixture gradients against true autograd with the log-joints recomputed: the rule of tests/test_gmm_backward.py."""
    return max(1e-4, 3.0 * floor)


def bar_lp(ref, floor_abs):
    """Log-joints and log p, absolute: max(2e-6 max|lp|, 4 x the fp32 CPU floor)."""
    return max(2e-6 * ref.abs().max().item(), 4.0 * floor_abs)


# ================================================================================================ context-shifted mixture
def gmm_ctx_group(N, MK):
    """(S, bytes of dynamic LDS) of the context-mixture kernels - a restatement of gmm_ctx_group in csrc/cf_context.hip: as
    many samples per workgroup (4, 2, 1) as fit 64 KiB with x of S samples and 5 S MK floats of log-joint scratch; S = 1 may
    take up to 160 KiB (the raised path), above that the call is refused (S = 0)."""
    for S in (4, 2, 1):
        lds = (S * N + 5 * S * MK) * 4
        if lds <= 64 * 1024:
            return S, lds
    return (1 if lds <= 160 * 1024 else 0), lds


def threshold_margin(N, MK):
    """Smallest relative distance of the shape's LDS need at S = 4, 2, 1 from the limits that pick the branch."""
    return min(abs((S * N + 5 * S * MK) * 4 - lim) / lim for S, lim in ((4, 65536), (2, 65536), (1, 65536), (1, 163840)))


def seg_lanes(HW):
    """SEG of GmmCtxLanes: the largest power of two <= min(64, HW)."""
    seg = 64
    while seg > HW:
        seg >>= 1
    return seg


def mixture_case(M, K, D, H, W, B, U, seed, Um=None):
    """Inputs of one mixture case, fp32, as _overlap_case of tests/test_gmm_backward.py scaled for N = D H W terms per
    log-joint: component means 1/sqrt(N) per element around a common centre, scales a relative 0.5/sqrt(N) apart, mean
    shifts of size 1/sqrt(N), scale shifts 0.3 randn per (key, mixture, channel) + 0.2/sqrt(N) per component (U distinct
    rows, picked by a key per sample: the table form), samples drawn from the shifted mixtures themselves.  Um: the mean
    shifts come from a table of Um rows too (cm_tab, ckey), as an embedding context net gives them."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    N = D * H * W
    rs = 1.0 / math.sqrt(N)
    mG = rn(M, 1, D, H, W) + rn(M, K, D, H, W) * rs
    sigma = (0.5 + torch.rand(M, 1, D, H, W, generator=gen)) * (1.0 + 0.5 * rn(M, K, D, H, W) * rs)
    sG = torch.log(torch.expm1(sigma))
    wG = rn(M, K)
    cs_tab = 0.3 * rn(U, M, 1, D) + 0.2 * rs * rn(U, M, K, D)
    key = torch.randint(0, U, (B,), generator=gen)
    cm_tab = ckey = None
    if Um is None:
        cm = rn(B, M, K, D) * rs
    else:
        cm_tab, ckey = rn(Um, M, K, D) * rs, torch.randint(0, Um, (B,), generator=gen)
        cm = cm_tab[ckey]
    c = torch.stack([cm, cs_tab[key].expand(B, M, K, D)], 1).contiguous()          # (B, 2, M, K, D)
    mb, kb = torch.randint(0, M, (B,), generator=gen), torch.randint(0, K, (B,), generator=gen)
    ar = torch.arange(B)
    mu = mG[mb, kb] + c[ar, 0, mb, kb].view(B, D, 1, 1)
    sig = F.softplus(sG[mb, kb] + c[ar, 1, mb, kb].view(B, D, 1, 1))
    x = mu + sig * rn(B, D, H, W)
    g = rn(B, M)
    return types.SimpleNamespace(M=M, K=K, D=D, H=H, W=W, B=B, U=U, N=N, x=x, mG=mG, sG=sG, wG=wG, logw=torch.log_softmax(wG.double(), -1).float(),
                                 c=c, cs_tab=cs_tab.reshape(U, M * K, D).contiguous(), key=key, g=g,
                                 cm_tab=None if cm_tab is None else cm_tab.reshape(Um, M * K * D), ckey=ckey)


def _terms(x, mG, sG, c):
    """d = x - mu - cm, s = sG + cs, sig = softplus(s), each (B, M, K, D, H, W)."""
    B, M, K, D = c.shape[0], c.shape[2], c.shape[3], c.shape[4]
    d = x.reshape(B, 1, 1, *x.shape[1:]) - mG.unsqueeze(0) - c[:, 0].reshape(B, M, K, D, 1, 1)
    s = sG.unsqueeze(0) + c[:, 1].reshape(B, M, K, D, 1, 1)
    return d, s, F.softplus(s)


def mixture_logjoints(x, mG, sG, logw, c):
    """lp (B, M, K): the per-component log-joints of oracle.flow_oracle.gmm_ctx_logprob, the shifts c (B, 2, M, K, D) given."""
    d, _, sig = _terms(x, mG, sG, c)
    return (-0.5 * (d / sig) ** 2 - torch.log(sig) - 0.5 * LOG_2PI).flatten(3).sum(-1) + logw


def mixture_autograd(case, dtype, chunk=64):
    """lp (B, M, K), out = logsumexp_k lp (B, M) and the gradients of sum(g * out) with respect to x and c, by torch.autograd
    in `dtype`, per chunk of samples."""
    t = lambda v: v.to(dtype)
    x, c = t(case.x).clone().requires_grad_(True), t(case.c).clone().requires_grad_(True)
    mG, sG, logw, g = t(case.mG), t(case.sG), torch.log_softmax(t(case.wG), -1), t(case.g)
    lps = []
    for b0 in range(0, case.B, chunk):
        lp = mixture_logjoints(x[b0:b0 + chunk], mG, sG, logw, c[b0:b0 + chunk])
        (torch.logsumexp(lp, -1) * g[b0:b0 + chunk]).sum().backward()
        lps.append(lp.detach())
    lp = torch.cat(lps, 0)
    return dict(lp=lp, out=torch.logsumexp(lp, -1), gx=x.grad, gc=c.grad)


def mixture_given_lp(case, lp, dtype, defect=None, S=None, chunk=64):
    """Closed form given the log-joints lp (B, M, K): r = g softmax_k(lp);
         gx = -sum_mk r d / sig^2;   gc[0] = sum_hw r d / sig^2;   gc[1] = sum_hw r (d^2 / sig^3 - 1 / sig) sigmoid(s);
         gmG, gsG = the summands of gc[0], gc[1] summed over the batch instead of the pixels.
    defect: "drop_last" (the last sample of a ragged group of S gets no gradient and joins no sum), "no_dsig" (softplus' missing),
    "second_pass" (the pixels of the first pass of 4 SEG are lost from gc: `=` where the second pass must `+=`)."""
    t = lambda v: v.to(dtype)
    x, c, mG, sG, g = t(case.x), t(case.c), t(case.mG), t(case.sG), t(case.g)
    r = torch.softmax(t(lp), -1) * g.unsqueeze(-1)
    if defect == "drop_last":
        assert case.B % S != 0
        r = r.clone()
        r[-1] = 0
    HW = case.H * case.W
    gx, gc0, gc1 = [], [], []
    gmG, gsG = torch.zeros_like(mG), torch.zeros_like(sG)
    for b0 in range(0, case.B, chunk):
        d, s, sig = _terms(x[b0:b0 + chunk], mG, sG, c[b0:b0 + chunk])
        rb = r[b0:b0 + chunk].reshape(-1, case.M, case.K, 1, 1, 1)
        q0 = rb * d / sig ** 2
        q1 = rb * (d ** 2 / sig ** 3 - 1.0 / sig) * (1.0 if defect == "no_dsig" else torch.sigmoid(s))
        gx.append(-q0.sum((1, 2)))
        gmG += q0.sum(0)
        gsG += q1.sum(0)
        if defect == "second_pass":
            first = 4 * seg_lanes(HW)
            assert HW > first
            q0, q1 = q0.flatten(4)[..., first:], q1.flatten(4)[..., first:]
        gc0.append(q0.flatten(4).sum(-1))
        gc1.append(q1.flatten(4).sum(-1))
    return dict(gx=torch.cat(gx, 0), gc=torch.stack([torch.cat(gc0, 0), torch.cat(gc1, 0)], 1), gmG=gmG, gsG=gsG)


def mixture_param_grads(case, r, dtype, slab=None, omit_slab=None, chunk=64):
    """gmG, gsG (M, K, D, H, W) given r (B, M K): sum_b r d / sig^2 and sum_b r (d^2 / sig^3 - 1 / sig) sigmoid(s).
    omit_slab: the partial of that slab of `slab` samples is left out (defect)."""
    t = lambda v: v.to(dtype)
    x, c, mG, sG = t(case.x), t(case.c), t(case.mG), t(case.sG)
    r = t(r).reshape(case.B, case.M, case.K).clone()
    if omit_slab is not None:
        r[omit_slab * slab:(omit_slab + 1) * slab] = 0
    gmG, gsG = torch.zeros_like(mG), torch.zeros_like(sG)
    for b0 in range(0, case.B, chunk):
        d, s, sig = _terms(x[b0:b0 + chunk], mG, sG, c[b0:b0 + chunk])
        rb = r[b0:b0 + chunk].reshape(-1, case.M, case.K, 1, 1, 1)
        gmG += (rb * d / sig ** 2).sum(0)
        gsG += (rb * (d ** 2 / sig ** 3 - 1.0 / sig) * torch.sigmoid(s)).sum(0)
    return dict(gmG=gmG, gsG=gsG)


# ================================================================================================ Conv1x1 / ActNorm with a context net
def affine_operands(C, HW, B, seed, trained=False, with_shared=True):
    """fp32 operands of one Conv1x1 / ActNorm case: x, gz (B, C, HW), gld (B) != 0, the per-sample CN(c) outputs m (B, C, C)
    and ma (B, 2 C), the shared Wm (C, C), t, logs (C) (None without them).  trained: diag(m) in +-3 and strictly-lower
    entries up to 1, as the CN nets of trained specialists give; otherwise m = 0.3 randn."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    x, gz = rn(B, C, HW), rn(B, C, HW)
    gld = rn(B)
    gld = torch.where(gld.abs() < 0.1, torch.full_like(gld, 0.7), gld)
    if trained:
        m = 2.0 * torch.rand(B, C, C, generator=gen) - 1.0
        m = torch.tril(m, -1) + torch.triu(rn(B, C, C), 1) + torch.diag_embed(6.0 * torch.rand(B, C, generator=gen) - 3.0)
    else:
        m = 0.3 * rn(B, C, C)
    ma = 0.3 * rn(B, 2 * C)
    Wm = t = logs = None
    if with_shared:
        Wm = torch.linalg.qr(rn(C, C))[0].contiguous()
        t, logs = 0.5 * rn(C), 0.3 * rn(C)
    return types.SimpleNamespace(C=C, HW=HW, B=B, x=x, gz=gz, gld=gld, m=m, ma=ma, Wm=Wm, t=t, logs=logs)


def conv1x1_ctx(x, m, Wm):
    """(z, ldj) of the formula of oracle.flow_oracle.conv1x1_ctx_fwd with m = CN(c) (B, C, C) given and logp_c = 0: W_b =
    tril(m, -1) + diag(exp(diag m)) [+ Wm - I]; ldj = H W sum diag m (without the constant H W log|det Wm|)."""
    diag = torch.diagonal(m, dim1=-2, dim2=-1)
    Wb = torch.tril(m, -1) + torch.diag_embed(torch.exp(diag))
    if Wm is not None:
        Wb = Wb - torch.eye(m.shape[-1], dtype=m.dtype) + Wm
    return Wb @ x, x.shape[-1] * diag.sum(-1)


def conv1x1_ctx_grads(o, dtype, defect=None):
    """gx (B, C, HW), gm (B, C, C) of sum(gz * z) + sum(gld * ldj) by autograd in `dtype`.  defect: "no_gld" (H W gld missing
    from the diagonal of gm), "diag_m" (the diagonal of W_b^T taken from m instead of exp(m) in the data gradient)."""
    t = lambda v: None if v is None else v.to(dtype)
    x, m = t(o.x).clone().requires_grad_(True), t(o.m).clone().requires_grad_(True)
    z, ldj = conv1x1_ctx(x, m, t(o.Wm))
    ((z * t(o.gz)).sum() + (ldj * t(o.gld)).sum()).backward()
    gx, gm = x.grad, m.grad
    if defect == "no_gld":
        gm = gm - o.HW * torch.diag_embed(t(o.gld).view(-1, 1).expand(-1, o.C))
    if defect == "diag_m":
        md = m.detach()
        Wb = torch.tril(md, -1) + torch.diag_embed(torch.diagonal(md, dim1=-2, dim2=-1))
        if o.Wm is not None:
            Wb = Wb - torch.eye(o.C, dtype=dtype) + t(o.Wm)
        gx = Wb.transpose(1, 2) @ t(o.gz)
    return dict(gx=gx, gm=gm)


def actnorm_ctx(x, ma, t, logs):
    """(z, ldj) of the formula of oracle.flow_oracle.actnorm_ctx_fwd with ma = CN(c) = [t_b | l_b] (B, 2 C) given, logp_c = 0."""
    C = x.shape[1]
    tb, lb = ma[:, :C], ma[:, C:]
    if t is not None:
        tb, lb = tb + t.view(1, -1), lb + logs.view(1, -1)
    return (x - tb.unsqueeze(-1)) * torch.exp(-lb.unsqueeze(-1)), lb.sum(-1)


def actnorm_ctx_grads(o, dtype):
    t = lambda v: None if v is None else v.to(dtype)
    x, ma = t(o.x).clone().requires_grad_(True), t(o.ma).clone().requires_grad_(True)
    z, ldj = actnorm_ctx(x, ma, t(o.t), t(o.logs))
    ((z * t(o.gz)).sum() + (ldj * t(o.gld)).sum()).backward()
    return dict(gx=x.grad, gm=ma.grad)
