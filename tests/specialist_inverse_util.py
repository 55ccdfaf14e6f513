"""Shared pieces of tests/test_specialist_inverse.py: the inverse problem a specialist fixture poses (the fp64 oracle's FORWARD
trace is the exact answer of every inverse), and a test-local torch restatement of the inverse chain of a specialist flow - the
per-sample matrix built as oracle.conv1x1_ctx_fwd builds it, the system solved with torch.linalg.solve - whose fp32 run on the CPU
is the floor the GPU bars rest on.  dtype-generic: fp64 parameters in, fp64 out."""
import functools
import types

import torch

from oracle import flow_oracle as fo
from tests.helpers import load_specialist

DEV = "cuda:0"
IDX9 = [0, 1, 2, 3, 0, 1, 2, 3, 1]
# the fixtures whose whole inverse chain the reference's own fp32 arithmetic can hold (per-sample matrices of condition <= 26);
# on the others (condition 2.3e2 .. 9.0e3) a plain fp32 restatement of the chain returns garbage: those are held per step
CHAIN_FIXTURES = ["mnist_eye_cf", "mnist_onehot", "cifar10_eye", "cifar10_eye_vardeq_cf", "cifar10_embed_eyesample",
                  "mnist_embed_probsample_cf", "cifar10_eye_argmax_cf"]
STEP_FIXTURES = CHAIN_FIXTURES + ["cifar10_onehot_cf", "smap_onehot_cf", "smap_eye", "atm_onehot_cf"]
CTX_KINDS = ("conv1x1", "actnorm", "coupling", "transcoupling")
PRE_KINDS = ("dequant", "affine", "logit", "augment")


def scale_of(ref):
    return max(1.0, ref.abs().max().item())


def err_of(got, ref):
    """max |got - ref| in units of the reference's scale."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return (got - ref).abs().max().item() / scale_of(ref)


def cast(params, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params.items()}


def codes(ops, params, ctx, context, cnoise, dtype):
    """{op position: (code, its log-density)} of every context layer, formed as flow_forward forms them: the encoders' noise is
    consumed in layer order."""
    cnoise = [c.to(dtype) for c in cnoise]
    et = ctx.get("enc_type", "uniform")
    out = {}
    for i, op in enumerate(ops):
        if op[0] not in CTX_KINDS:
            continue
        pre = "%d.context_net.1." % op[1]
        if et == "vardeq":
            out[i] = fo.ctx_encode_vardeq(context, ctx, params, pre, cnoise.pop(0))
        elif et == "argmax":
            out[i] = fo.ctx_encode_argmax(context, ctx, params, pre, cnoise.pop(0))
        elif et == "probsample":
            out[i] = fo.ctx_encode_probsample(context, ctx, params, pre, cnoise.pop(0))
        elif et == "eyesample":
            w = [params["%d.context_net.0._embeddings.%d.weight" % (op[1], j)] for j in range(len(ctx["contexts"]))]
            out[i] = (torch.cat([w[j][context[:, j]] for j in range(len(w))], 1), torch.zeros(context.shape[0], dtype=dtype))
        else:
            out[i] = fo.ctx_encode(context, ctx, cnoise.pop(0))
    assert not cnoise
    return out


def sample_matrix(params, pre, c, contextflow, D):
    """W_b of a context Conv1x1, as oracle.conv1x1_ctx_fwd builds it."""
    m = (c @ params[pre + "CN.weight"].t() + params[pre + "CN.bias"]).reshape(c.shape[0], D, D)
    diag = torch.diagonal(torch.tril(m), dim1=-2, dim2=-1)
    tri = torch.tril(m, diagonal=-1) + torch.diag_embed(torch.exp(diag))
    if contextflow:
        tri = tri - torch.eye(D, dtype=c.dtype) + params[pre + "NN"]
    return tri


def conv1x1_ctx_inv(z, params, pre, c, contextflow):
    B, D, H, W = z.shape
    return torch.linalg.solve(sample_matrix(params, pre, c, contextflow, D), z.reshape(B, D, H * W)).reshape(B, D, H, W)


def actnorm_ctx_inv(z, params, pre, c, contextflow):
    B, D = z.shape[:2]
    m = c @ params[pre + "CN.weight"].t() + params[pre + "CN.bias"]
    tb, lb = m[:, :D], m[:, D:]
    if contextflow:
        tb, lb = tb + params[pre + "NN_t"].view(1, -1), lb + params[pre + "NN_logs"].view(1, -1)
    return z * torch.exp(lb.view(B, D, 1, 1)) + tb.view(B, D, 1, 1)


def ctx_op_inverse(op, params, ctx, code, z):
    """The inverse of one context layer on its forward output z."""
    kind, pre, cf = op[0], "%d." % op[1], ctx["contextflow"]
    c = code[0]
    if kind == "conv1x1":
        return conv1x1_ctx_inv(z, params, pre, c, cf)
    if kind == "actnorm":
        return actnorm_ctx_inv(z, params, pre, c, cf)
    B, C, H, W = z.shape
    z0 = z[:, : C // 2]
    cn = fo.coupling_cn(c, params, pre)
    wide = lambda: torch.cat([z0, cn.view(B, -1, 1, 1).expand(B, cn.shape[1], H, W)], 1)
    if kind == "coupling":
        h = fo.coupling_net(z0, params, pre, op[4]) + cn.view(B, -1, 1, 1) if cf else fo.coupling_net(wide(), params, pre, op[4])
    else:
        h = (fo.vit_net(z0, params, pre, op[2], op[3]) + cn.view(B, -1, 1, 1) if cf
             else fo.vit_net(wide(), params, pre, op[2], op[3], concat=True))
    return fo.coupling_apply_inv(z, h)


def first_flow_op(ops):
    """Position of the first op behind the pre-processing (Dequantization .. LogitTransform [, Augment])."""
    i = 0
    while i < len(ops) and ops[i][0] in PRE_KINDS:
        i += 1
    return i


def spec_inverse(ops, params, ctx, code, z, halves, first):
    """The reverse chain of a specialist program from (z, halves in forward order) back to the tensor that entered ops[first]."""
    halves = list(halves)
    for i in range(len(ops) - 1, first - 1, -1):
        op = ops[i]
        if op[0] in CTX_KINDS:
            z = ctx_op_inverse(op, params, ctx, code[i], z)
        elif op[0] == "split":
            z = torch.cat([z, halves.pop().to(z.dtype)], 1)
        else:
            z = fo.flow_inverse([op], params, z)
    assert not halves
    return z


@functools.lru_cache(maxsize=None)
def problem(fxname, B=4, u_half=False):
    """One (fixture, batch): the fixture's rows, contexts and encoder noise through the fp64 oracle with a trace.  u_half: the
    dequantisation noise pinned to 0.5 (the pixel tests).  Computed once and shared; nobody writes into it."""
    name, ctx, ops, M, params, inp = load_specialist(fxname)
    idx = torch.tensor({4: [0, 1, 2, 3], 9: IDX9}[B])
    rows = lambda t: t[idx] if t.shape[0] == inp["x"].shape[0] else t
    x, u, context = rows(inp["x"]), rows(inp["u"]), rows(inp["context"])
    if u_half:
        u = torch.full_like(u, 0.5)
    eps, cnoise = [rows(e) for e in inp["eps"]], [rows(c) for c in inp["cnoise"]]
    p64 = cast(params, torch.float64)
    tr = []
    x64 = x.double()
    _, lp = fo.flow_forward(ops, p64, x64, u.double(), [e.double() for e in eps], trace=tr, ctx=ctx, context=context,
                            cnoise=[c.double() for c in cnoise])
    z, halves, inputs = fo.inverse_problem(ops, x64, tr)
    return types.SimpleNamespace(fxname=fxname, name=name, ctx=ctx, ops=ops, M=M, params=params, x=x, u=u, eps=eps, context=context,
                                 cnoise=cnoise, z=z, halves=halves, inputs=inputs, lp=lp, first=first_flow_op(ops))


@functools.lru_cache(maxsize=None)
def chain_floor(fxname, B=4, u_half=False):
    """(error of the fp32 restatement of the chain against the trace in front of the pre-processing, of scale; the pixels its
    continuation through the pre-processing returns)."""
    p = problem(fxname, B, u_half)
    p32 = cast(p.params, torch.float32)
    code = codes(p.ops, p32, p.ctx, p.context, p.cnoise, torch.float32)
    y = spec_inverse(p.ops, p32, p.ctx, code, p.z.float(), [h.float() for h in p.halves], p.first)
    pix = fo.flow_inverse(p.ops[:p.first], p32, y)
    return err_of(y, p.inputs[p.first]), pix


def ctx_pairs(ops):
    """[(position of the conv1x1, a Squeeze((2,2)) sits in front of it)] of every Conv1x1 -> ActNorm pair."""
    out = []
    for i in range(len(ops) - 1):
        if ops[i][0] == "conv1x1" and ops[i + 1][0] == "actnorm":
            out.append((i, i > 0 and ops[i - 1][0] == "squeeze" and tuple(ops[i - 1][2]) == (2, 2)))
    return out


def build_specialist(p, u=None, eps=None):
    """The flow of a problem on the device, evaluation mode, frozen; u / eps: the pre-processing's noise (tests.gpu_util.set_noise)."""
    import contextflow_amd as cfa
    from tests.gpu_util import set_noise
    cfg, ds, MM = cfa.preset_config(p.name)
    cfg.update(generalist=False, enc_emb=p.ctx["enc_emb"], enc_type=p.ctx.get("enc_type", "uniform"), contextflow=p.ctx["contextflow"])
    model = cfa.create_model(cfg, ds, MM, contexts=p.ctx["contexts"])
    model.load_state_dict({k: v.clone() for k, v in p.params.items()}, strict=True)
    model = model.to(DEV).eval()
    for q in model.parameters():
        q.requires_grad_(False)
    set_noise(model, u, eps if eps is not None else [])
    return model


def fixture_noise(p):
    """The fixture's encoder noise in the form `noise=` takes: one tensor per stochastic encoder, in layer order."""
    return [c.to(DEV) for c in p.cnoise]


def affine_inv_ref(z, m1, Wm, m2, t, logs, dtype=torch.float64):
    """x = W_b^-1 (z exp(l_b) + t_b) per pixel in `dtype` on the CPU: the formula cf_affine_ctx_inv computes."""
    B, C = z.shape[:2]
    d = lambda v: None if v is None else v.to(dtype)
    y = d(z).reshape(B, C, -1)
    if m2 is not None:
        tb, lb = d(m2)[:, :C], d(m2)[:, C:]
        if logs is not None:
            tb, lb = tb + d(t), lb + d(logs)
        y = y * torch.exp(lb)[:, :, None] + tb[:, :, None]
    if m1 is not None:
        M1 = d(m1).view(B, C, C)
        Wb = torch.tril(M1, -1) + torch.diag_embed(torch.exp(torch.diagonal(M1, dim1=1, dim2=2)))
        if Wm is not None:
            Wb = Wb + d(Wm) - torch.eye(C, dtype=dtype)
        y = torch.linalg.solve(Wb, y)
    return y.reshape(z.shape)
