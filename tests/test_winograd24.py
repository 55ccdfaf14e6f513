"""The Winograd F(2x4, 3x3) form of the coupling nets' 3x3 on the 4x4 level (contextflow_amd/csrc/cf_step_common.h:
winograd24_phase2): F(2, 3) down the rows, F(4, 3) on the points {0, 1, -1, 1/2, -1/2, inf} along the columns.  CPU: the
transforms, a restatement of the form in fp32 against the fp64 direct convolution, and the end-to-end fixtures through the
oracle with the 4x4 level's 3x3 in this form.  GPU: the production step kernel against the oracle, and the tiled fixtures."""

import pytest
import torch
import torch.nn.functional as F

from oracle import flow_oracle as fo
from oracle.winograd import winograd3x3_reflect
from tests.helpers import load_e2e, e2e_inputs, bpd, stress_tolerance

BPD_TOL = 1e-5
DEV = "cuda:0"

# U = G2 w G4^T (fp64, rounded once: k_step_pack), V = B2^T d B4, Y = A2^T M A4
G2 = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
G4 = torch.tensor([[4, 0, 0], [2 / 3, 2 / 3, 2 / 3], [2 / 3, -2 / 3, 2 / 3], [-8 / 3, -4 / 3, -2 / 3], [-8 / 3, 4 / 3, -2 / 3],
                   [0, 0, 1]], dtype=torch.float64)
BT2 = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float32)
BT4 = torch.tensor([[.25, 0, -1.25, 0, 1, 0], [0, -.25, -.25, 1, 1, 0], [0, .25, -.25, -1, 1, 0], [0, -.5, -1, .5, 1, 0],
                    [0, .5, -1, -.5, 1, 0], [0, .25, 0, -1.25, 0, 1]], dtype=torch.float32)
AT2 = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float32)
AT4 = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, .5, -.5, 0], [0, 1, 1, .25, .25, 0], [0, 1, -1, .125, -.125, 1]],
                   dtype=torch.float32)


def winograd24_3x3_reflect(h, w, b):
    """h (B, Ci, H, W) fp32, w (Co, Ci, 3, 3), b (Co,) -> conv2d(reflect_pad(h, 1), w) + b; H even, W a multiple of 4.
    The kernel's order: vertical transform per patch column, horizontal transform, per-position contraction with fp32
    accumulation, output transform."""
    B, Ci, H, W = h.shape
    U = torch.einsum("xa,oiab,yb->xyoi", G2, w.double(), G4).float()                 # (4, 6, Co, Ci), rounded once
    d = F.pad(h, (1, 1, 1, 1), mode="reflect").unfold(2, 4, 2).unfold(3, 6, 4)       # (B, Ci, H/2, W/4, 4, 6) input patches
    V = torch.einsum("xa,ncijab->ncijxb", BT2, d)
    V = torch.einsum("ncijxb,yb->ncijxy", V, BT4)
    M = torch.einsum("xyoc,ncijxy->noijxy", U, V)
    Y = torch.einsum("noijxy,qy->noijxq", M, AT4)
    Y = torch.einsum("px,noijxq->noijpq", AT2, Y)                                     # (B, Co, H/2, W/4, 2, 4)
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(B, -1, H, W) + b.view(1, -1, 1, 1)


def coupling_net_production(x0, p, prefix, pad):
    """oracle.flow_oracle.coupling_net with the 3x3 in the forms the evaluation forward runs at saturating batches:
    F(2x4, 3x3) on 4x4 images, F(2x2, 3x3) elsewhere."""
    h = F.relu(F.conv2d(x0, p[prefix + "NN.0.weight"], p[prefix + "NN.0.bias"]))
    assert h.dtype == torch.float32 and tuple(pad) == (1, 1)
    conv = winograd24_3x3_reflect if h.shape[2:] == (4, 4) else winograd3x3_reflect
    h = F.relu(conv(h, p[prefix + "NN.2.weight"], p[prefix + "NN.2.bias"]))
    return F.conv2d(h, p[prefix + "NN.4.weight"], p[prefix + "NN.4.bias"])


def test_the_one_dimensional_transforms_are_exact():
    """A4^T [(G4 g) * (B4^T d)] is the correlation of d (6) with g (3) in exact arithmetic, and so for F(2, 3); every B / A
    entry is a short binary fraction (exact in fp32)."""
    g = torch.randn(3, 50, dtype=torch.float64)
    for AT, Gm, BT, m in ((AT4, G4, BT4, 4), (AT2, G2, BT2, 2)):
        d = torch.randn(m + 2, 50, dtype=torch.float64)
        got = AT.double() @ ((Gm @ g) * (BT.double() @ d))
        want = torch.stack([(d[i:i + 3] * g).sum(0) for i in range(m)])
        assert (got - want).abs().max().item() < 1e-12
        for t in (AT, BT):
            assert torch.equal((t * 8).round(), t * 8)


@pytest.mark.parametrize("H,W", [(4, 4), (8, 8), (16, 16)])
def test_restatement_against_the_fp64_direct_convolution(H, W):
    torch.manual_seed(H)
    Ci = Co = 64
    h = torch.relu(torch.randn(8, Ci, H, W))
    w, b = 0.05 * torch.randn(Co, Ci, 3, 3), 0.1 * torch.randn(Co)
    ref = F.conv2d(F.pad(h.double(), (1, 1, 1, 1), mode="reflect"), w.double(), b.double())
    direct32 = F.conv2d(F.pad(h, (1, 1, 1, 1), mode="reflect"), w, b)
    got = winograd24_3x3_reflect(h, w, b)
    scale = ref.abs().max().item()
    err, err_direct = (got.double() - ref).abs().max().item(), (direct32.double() - ref).abs().max().item()
    # the half-point form carries a few times the direct sum's rounding, far below the bars of the step tests (1e-5 of scale)
    assert err <= 4e-6 * scale and err <= 16 * max(err_direct, 1e-7 * scale), (err, err_direct, scale)


@pytest.mark.parametrize("tag", [None, "stress", "extreme"])
def test_e2e_fixtures_with_the_2x4_form_on_the_4x4_level(tag):
    """The oracle's flow on the reference's cifar10 end-to-end fixtures (mnist's flow has no 4x4 level) with the 3x3 in the
    production forms (F(2x4) on 4x4 images, F(2x2) elsewhere, fp32): bits/dim within the 1e-5 bar of the reference's fp32
    and fp64 results in every regime."""
    name = "cifar10"
    ops, _, M, params, fx = load_e2e(name, tag)
    x, u, eps = e2e_inputs(name, fx)
    tol = stress_tolerance(fx, tag) if tag else BPD_TOL
    direct, calls = fo.coupling_net, []

    def counted(x0, p, prefix, pad):
        calls.append(tuple(x0.shape[2:]))
        return coupling_net_production(x0, p, prefix, pad)
    try:
        fo.coupling_net = counted
        _, logp = fo.flow_forward(ops, params, x, u, eps)
    finally:
        fo.coupling_net = direct
    assert calls.count((4, 4)) == 4, calls          # the four couplings of the 4x4 level took the F(2x4) form
    assert (bpd(logp, name) - bpd(torch.from_numpy(fx["logp"]), name)).abs().max().item() < tol
    if "logp_f64" in fx:
        assert (bpd(logp, name) - bpd(torch.from_numpy(fx["logp_f64"]), name)).abs().max().item() < tol


@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


@pytest.mark.gpu
@pytest.mark.parametrize("squeeze", [False, True])
@pytest.mark.parametrize("C,H", [(16, 16), (32, 8), (64, 4)])
def test_production_step_kernel_at_a_saturating_batch(L, C, H, squeeze):
    """One fused step through the production entry point at 4100 samples (the 4x4 level: the F(2x4) kernel; the last
    workgroup partially filled), against the fp64 oracle of the step and against the direct-form kernel: z to 1e-5 of its
    scale, the log-det to 1e-5 relative."""
    from tests.gpu_util import fused_step_debug
    from contextflow_amd.layers import _hip
    B, W = 4100, H
    if (C, H) == (64, 4):      # the dispatch takes the F(2x4) form here: 16 instead of 20 C^2 HW multiply-adds per step
        per_px = 16
        assert _hip.lib().cf_flow_step_macs(B, C, H, W, 0) == per_px * C * C * H * W
    torch.manual_seed(C * 1000 + 7)                      # the parameters of test_winograd_step_kernel_against_the_oracle
    conv, act, cpl = L.Conv1x1((C, H, W)), L.ActNorm((C, H, W)), L.Coupling(C, kernel_size=(3, 3), padding=(1, 1))
    with torch.no_grad():
        conv.NN.add_(0.1 * torch.randn(C, C))
        act.NN_t.copy_(0.3 * torch.randn(C)); act.NN_logs.copy_(0.2 * torch.randn(C)); act.initialized.fill_(1)
    act._init_done = True
    x = torch.randn(B, C, H, W)
    p = {"0." + k: v.detach().double() for k, v in cpl.state_dict().items()}
    y, l0 = fo.conv1x1_fwd(x.double(), conv.NN.detach().double())
    y, l1 = fo.actnorm_fwd(y, act.NN_t.detach().double(), act.NN_logs.detach().double())
    zref, l2 = fo.coupling_fwd(y, p, "0.", (1, 1))
    for m in (conv, act, cpl):
        m.to(DEV)
    xin = fo.squeeze_inv(x, (2, 2)) if squeeze else x
    z, ldj, d = fused_step_debug(xin.to(DEV).contiguous(), conv, act, cpl, squeeze=squeeze)
    scale = max(1.0, zref.abs().max().item())
    for got in (d["z_prod"], z):
        assert (got.cpu().double() - zref).abs().max().item() <= 1e-5 * scale
    lref = l0 + l1 + l2
    for got in (d["ldj_prod"], ldj):
        assert ((got.cpu().double() - lref).abs() / lref.abs().clamp_min(1.0)).max().item() <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("tag", [None, "stress", "extreme"])
def test_cifar10_fixtures_tiled_to_4096_samples(L, tag):
    """The cifar10 fixtures' samples and captured noise repeated to 4096 rows through the evaluation forward (no autograd:
    with gradients the fused plan takes the taping kernels, which keep F(2x2)): the 4x4 level's steps run the F(2x4) kernel
    and every row reproduces the reference's log-density within the end-to-end bars."""
    from tests.gpu_util import build_model, set_noise
    from contextflow_amd.layers import _hip
    name = "cifar10"
    ops, _, M, params, fx = load_e2e(name, tag)
    x, u, eps = e2e_inputs(name, fx)
    rep = 4096 // x.shape[0]
    B = x.shape[0] * rep
    tol = stress_tolerance(fx, tag) if tag else BPD_TOL
    model = build_model(name, params)
    set_noise(model, u.repeat(rep, 1, 1, 1), [e.repeat(rep, *([1] * (e.dim() - 1))) for e in eps])
    model.step_events = []            # (start, end, batch, C, H*W) per cf_flow_step_fwd launch
    try:
        with torch.no_grad():
            z, logp = model(x.repeat(rep, 1, 1, 1).to(DEV))
        torch.cuda.synchronize()
        launches = [(e[2], e[3], e[4]) for e in model.step_events]
    finally:
        model.step_events = None
    # the 4x4 level's steps went through cf_flow_step_fwd at this batch, and its dispatch there is the F(2x4) kernel
    assert launches.count((B, 64, 16)) == 4, launches
    per_px = 16
    assert _hip.lib().cf_flow_step_macs(B, 64, 4, 4, 0) == per_px * 64 * 64 * 16
    lp = logp.cpu()
    for key in ("logp", "logp_f64"):
        if key in fx:
            ref = torch.from_numpy(fx[key]).repeat(rep, 1)
            assert (bpd(lp, name) - bpd(ref, name)).abs().max().item() < tol, key
    zr = torch.from_numpy(fx["z"]).repeat(rep, 1, 1, 1)
    assert (z.cpu() - zr).abs().max().item() <= 2e-4 * max(1.0, zr.abs().max().item())
