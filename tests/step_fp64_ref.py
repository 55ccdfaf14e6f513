"""CPU side of tests/test_step_backward_fp64.py: the cases, their inputs, and one fused conv flow step
([Squeeze ->] Conv1x1 -> ActNorm -> Coupling, optionally with the specialist's per-sample bias) written over
oracle/flow_oracle.py with the two ReLUs as `a * m`, so that a run can be given the masks of another run.

Why masks are imposed: a ReLU unit whose pre-activation lies within fp32 rounding of zero gets the other mask bit in another
summation order.  At C = 16, 16x16, B = 259 one such unit out of 4.2 M moves dL/dx by 8.5e-3 of its largest entry and the
gradient of NN.0.weight by 7.7e-4 between fp32 and fp64 torch.autograd - both correct.  With the masks of one run imposed on the
other the same pair agrees to 1.5e-7 (dL/dx) .. 1.4e-6 (biases).  So the test checks "which side of zero" on its own (a mask may
differ from the fp64 run's only where |a| < TAU max(1, |a|), and the inputs must keep the share of such units under BAND_MAX),
the planes and outputs against the true-ReLU run, and the gradients under the kernel's masks.

Nothing here touches a GPU: tests/test_step_backward_fp64.py::test_reference_* run it on the CPU."""
from typing import NamedTuple

import torch
import torch.nn.functional as F

from oracle import flow_oracle as fo

TAU = 1e-5               # half-width of the band around zero in which a mask bit may differ: ~10 fp32 roundings of these sums
BAND_MAX = 1e-4          # largest share of ReLU units the inputs may put inside the band
GRAD_CAP = 1e-4          # the project's gradient bar
GRAD_MIN = 2e-6          # what two accumulation orders of these planes are allowed to differ by
FLOOR_FACTOR = 4.0       # Winograd forms (1.6x the direct sum's error) and the split-K order

PARAMS = ("Conv1x1.NN", "ActNorm.NN_t", "ActNorm.NN_logs", "NN.0.weight", "NN.0.bias", "NN.2.weight", "NN.2.bias", "NN.4.weight",
          "NN.4.bias")


class Case(NamedTuple):
    C: int
    H: int
    B: int
    squeeze: int = 0         # 1: x / gx are in the layout in front of the step's Squeeze((2,2))
    sliced: int = 0          # 1: x is the channel slice big[:, :c] of a tensor with twice the channels (batch stride 2 c h w)
    mode: int = 0            # 0: generalist; 1: sbias (B, C) on the conditioner output; 2: sbias (B, 2C) in front of the first ReLU
    seed: int = 0

    @property
    def id(self):
        return "C%d-H%d-B%d%s%s%s" % (self.C, self.H, self.B, "-sq" if self.squeeze else "", "-slice" if self.sliced else "",
                                      "-mode%d" % self.mode if self.mode else "")


# seeds other than 0: a draw of so few units (4096 at C = 64, B = 1) that ONE of them inside the band exceeds BAND_MAX
_SEED = {(64, 1, 0): 1}


def _generalist():
    # batch sizes: the smallest that reach each branch of the dispatch (cf_step_dispatch.h select(Pass::Taped, ...), cf_step_bwd.h
    # launch_bwd under cf_flow_step_bwd_taped) with a ragged last workgroup, and both sides of every threshold
    levels = [
        (8, 16, [3, 67]),                    # Small_G8s / B8 at every batch: one sample per workgroup, two sizes of grid
        (16, 16, [3, 67]),                   # Small_G16w (Winograd) / B16
        (32, 8, [5,                          # Rs_G32
                 512, 513,                   # kRsMaxB8x8 = 512: Rs_G32 | Step_G32v2
                 1023, 1027]),               # kFullMinB8x8 = 1024: Step_G32v2 | Step_G32w (Winograd); 1027: ragged B32 pair
        (64, 4, [1, 7,                       # Rs16_G64 / k_flow_step_bwd_rs16
                 1024, 1025,                 # kRs16MaxB4x4 = 1024: Rs16_G64 | Step_G64v2
                 1536, 1537,                 # CF_BWD_RS16_MAXB = 1536: k_flow_step_bwd_rs16 | B64 (8 samples / workgroup)
                 2047, 2051]),               # kWinoMinB4x4 = 2048: Step_G64v2 | Step_G64w2 (Winograd); 2051: ragged B64 tile
    ]
    out = []
    for C, H, Bs in levels:
        for sq in (0, 1):
            for i, B in enumerate(Bs):
                # the SplitPrior case (x = a channel slice, read in place by the Conv1x1 weight gradient): one per level and
                # layout, at the first batch with more than one workgroup in every kernel of the level
                out.append(Case(C, H, B, sq, int(i == 1), seed=_SEED.get((C, B, sq), 0)))
    return out


GENERALIST = _generalist()
# specialist twins.  Mode 2 (taped): the 16-sample forward's tape into rs16 (B = 19) and into the 8-sample tile backward (B = 1541 >
# CF_BWD_RS16_MAXB).  Mode 1 (recompute): two or more workgroups and a ragged last one at every level of k_flow_step_bwd<..., CTX>;
# the seeds are those for which the fp64 run has NO unit inside the band (the kernel's masks cannot be read back there)
MODE2 = [Case(8, 16, 3, mode=2), Case(16, 16, 3, mode=2), Case(32, 8, 7, mode=2), Case(64, 4, 19, mode=2), Case(64, 4, 1541, mode=2)]
MODE1 = [Case(8, 16, 3, mode=1, seed=4), Case(16, 16, 3, mode=1, seed=0), Case(32, 8, 7, mode=1, seed=0),
         Case(64, 4, 19, mode=1, seed=1)]
CASES = GENERALIST + MODE2 + MODE1


def draw(case):
    """fp32 CPU tensors of a case: parameters as tests/test_gpu_parity.py::test_step_backward_writes_the_unsqueezed_gradient draws
    them, x in the layout the kernel is handed (in front of the Squeeze if case.squeeze; `big` = the tensor it is a slice of, or
    None), gz, gld, and sbias for the specialist modes (whose Conv1x1 / ActNorm in front are the identity: no entry)."""
    C, H, B = case.C, case.H, case.B
    HID, HALF = 2 * C, C // 2
    g = torch.Generator().manual_seed(1000003 * case.seed + 7919 * C + 31 * B + 2 * case.mode + case.squeeze)
    r = lambda *sh: torch.randn(*sh, generator=g)
    p = {}
    if not case.mode:
        p["Conv1x1.NN"] = torch.linalg.qr(r(C, C))[0].contiguous()
        p["ActNorm.NN_t"], p["ActNorm.NN_logs"] = 0.1 * r(C), 0.1 * r(C)
    p["NN.0.weight"], p["NN.0.bias"] = 0.2 * r(HID, HALF, 1, 1), 0.1 * r(HID)
    p["NN.2.weight"], p["NN.2.bias"] = 0.05 * r(HID, HID, 3, 3), 0.1 * r(HID)
    p["NN.4.weight"], p["NN.4.bias"] = 0.05 * r(C, HID, 1, 1), 0.1 * r(C)
    shape = (C // 4, 2 * H, 2 * H) if case.squeeze else (C, H, H)
    big = None
    if case.sliced:
        big = r(B, 2 * shape[0], *shape[1:])
        x = big[:, :shape[0]]
    else:
        x = r(B, *shape)
    d = dict(p=p, x=x, big=big, gz=r(B, C, H, H), gld=r(B), sbias=None)
    if case.mode:
        d["sbias"] = 0.3 * r(B, C if case.mode == 1 else HID)
    return d


class _Gate(torch.autograd.Function):
    """a * mf forward, g * mb backward: a backward that reads ANOTHER mask than the forward used (test_defects_* only)."""
    @staticmethod
    def forward(ctx, a, mf, mb):
        ctx.save_for_backward(mb)
        return a * mf

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


def step_ref(d, squeeze=0, mode=0, m1=None, m2=None, dtype=torch.float64, grads=True, bwd_masks=None):
    """One step at `dtype` on the CPU from the tensors of draw(): every input and parameter a leaf, the ReLUs as a * m with m1 / m2
    (B, 2C, H, W) bool, None = the true ReLU (a > 0).  Loss = (z gz).sum() + (ld gld).sum().  Quirks as the oracle has them:
    ActNorm's ldj = +sum(logs), log_s = 2 tanh(raw / 2).  bwd_masks = (mb1, mb2): the backward multiplies by these
    instead (a restated defect; never set by the comparison with the kernels).  Returns a dict: z, ld, y0, h1, h2, a1, a2 (detached), and with grads:
    gx (layout of x), one entry per parameter name, gsbias."""
    lv = lambda t: t.detach().to(dtype).clone().requires_grad_(grads)
    p = {k: lv(v) for k, v in d["p"].items()}
    x = lv(d["x"])
    sb = lv(d["sbias"]) if mode else None
    gz, gld = d["gz"].to(dtype), d["gld"].to(dtype)
    y = fo.squeeze_fwd(x, (2, 2)) if squeeze else x
    B, C = y.shape[:2]
    ld = torch.zeros(B, dtype=dtype)
    if "Conv1x1.NN" in p:
        y, l0 = fo.conv1x1_fwd(y, p["Conv1x1.NN"])
        y, l1 = fo.actnorm_fwd(y, p["ActNorm.NN_t"], p["ActNorm.NN_logs"])
        ld = ld + l0 + l1
    y0 = y[:, : C // 2]
    a1 = F.conv2d(y0, p["NN.0.weight"], p["NN.0.bias"])
    if mode == 2:
        a1 = a1 + sb.view(B, -1, 1, 1)
    gate = lambda a, m, k: a * m if bwd_masks is None else _Gate.apply(a, m, bwd_masks[k].to(dtype))
    h1 = gate(a1, (a1.detach() > 0 if m1 is None else m1).to(dtype), 0)
    a2 = F.conv2d(F.pad(h1, (1, 1, 1, 1), mode="reflect"), p["NN.2.weight"], p["NN.2.bias"])
    h2 = gate(a2, (a2.detach() > 0 if m2 is None else m2).to(dtype), 1)
    h = F.conv2d(h2, p["NN.4.weight"], p["NN.4.bias"])
    if mode == 1:
        h = h + sb.view(B, -1, 1, 1)
    z, l2 = fo.coupling_apply_fwd(y, h)
    ld = ld + l2
    out = {k: v.detach() for k, v in dict(z=z, ld=ld, y0=y0, h1=h1, h2=h2, a1=a1, a2=a2).items()}
    if grads:
        ((z * gz).sum() + (ld * gld).sum()).backward()
        out["gx"] = x.grad
        out.update({k: v.grad for k, v in p.items()})
        if mode:
            out["gsbias"] = sb.grad
    return out


def grad_names(mode=0):
    if mode == 1:
        return ("gx", "gsbias")                  # the conditioner is frozen under contextflow
    return ("gx",) + (PARAMS if not mode else PARAMS[3:] + ("gsbias",))


def in_band(a):
    a = a.abs()
    return a < TAU * a.clamp(min=1.0)


def band_share(ref):
    """Share of the ReLU units of a true-ReLU fp64 run (step_ref) inside the band, per layer and overall, and their count."""
    n1, n2 = int(in_band(ref["a1"]).sum()), int(in_band(ref["a2"]).sum())
    return n1 / ref["a1"].numel(), n2 / ref["a2"].numel(), (n1 + n2) / (ref["a1"].numel() + ref["a2"].numel()), n1 + n2


def mask_disagreements(ref, m1, m2):
    """(number of units whose mask differs from the fp64 run's, number of those OUTSIDE the band)."""
    n = bad = 0
    for a, m in ((ref["a1"], m1), (ref["a2"], m2)):
        diff = (a > 0) != m.reshape(a.shape)
        n += int(diff.sum())
        bad += int((diff & ~in_band(a)).sum())
    return n, bad


def rel_err(got, ref):
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3)


def bar(floor):
    return min(GRAD_CAP, max(GRAD_MIN, FLOOR_FACTOR * floor))


def floors(d, case, m1, m2, ref=None):
    """Per tensor: the error of fp32 torch.autograd on the CPU on the same graph under the same imposed masks, against the fp64
    run under them (`ref`, computed if not given).  Returns (ref, {name: floor})."""
    if ref is None:
        ref = step_ref(d, case.squeeze, case.mode, m1, m2)
    r32 = step_ref(d, case.squeeze, case.mode, m1, m2, dtype=torch.float32)
    return ref, {k: rel_err(r32[k], ref[k]) for k in grad_names(case.mode)}
