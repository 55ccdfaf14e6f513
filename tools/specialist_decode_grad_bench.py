#!/usr/bin/env python3
"""Time of `decode(latents, context, differentiable=True)` + backward of a specialist flow (the latent gradient of the backward walk
under a context) next to the plain `decode(latents, context)` and to `score(x, context=c)` - in ONE process,
interleaved call by call - and of the three kernels of that walk next to their twins at the three image levels.

usage: specialist_decode_grad_bench.py [--cases cifar10_onehot_cf:8192,cifar10_onehot_cf:256,mnist_eye_cf:8192,mnist_eye_cf:256]
                                       [--iters 20] [--warmup 5] [--kernels B]

Per case one JSON line: medians (and min / max) of HIP-event times per call after the warm-up calls.  --kernels B, per level and B
samples, interleaved:
  cf_flow_step_inv_ctx next to cf_flow_step_inv (the generalist's step: one more 1x1 phase, no bias) and next to the layer-by-layer
  Coupling.reverse(z, c) it replaces inside this walk - both with the coupling's CN chain, as the walk runs them;
  cf_flow_step_inv_bwd_ctx_data next to cf_flow_step_bwd_ctx_data (the same recompute);
  cf_affine_ctx_inv_bwd_data next to cf_affine_ctx_inv (the same elimination)."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import contextflow_amd as cfa
from contextflow_amd.layers import _hip
from contextflow_amd.layers.autograd_inverse import _coupling_ctx_inverse
from contextflow_amd.layers.coupling import Coupling

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="cifar10_onehot_cf:8192,cifar10_onehot_cf:256,mnist_eye_cf:8192,mnist_eye_cf:256")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--kernels", type=int, default=0)
args = ap.parse_args()
dev = "cuda:0"
CONTEXTS = {"mnist": [64], "cifar10": [15, 5]}


def make(label):
    """(model, data(n), context(n)) of a specialist case, e.g. cifar10_onehot_cf (tools/specialist_sample_bench.py::make)."""
    kinds = label.split("_")
    name, spec = kinds[0], kinds[1:]
    torch.manual_seed(0)
    cfg, ds, M = cfa.preset_config(name)
    cf = spec[-1] == "cf"
    enc = spec[:-1] if cf else spec
    cfg.update(generalist=False, enc_emb=enc[0], enc_type=enc[1] if len(enc) > 1 else "uniform", contextflow=cf)
    model = cfa.create_model(cfg, ds, M, contexts=CONTEXTS[name]).to(dev)
    data = lambda n: torch.randint(0, 256, (n, *ds), device=dev).float()
    ctx = lambda n: torch.stack([torch.randint(0, k, (n,), device=dev) for k in CONTEXTS[name]], dim=1)
    with torch.no_grad():
        model(data(256), ctx(256))        # ActNorm init
    model.eval()
    for q in model.parameters():
        q.requires_grad_(False)
    return model, data, ctx


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def interleaved(calls, iters, warmup):
    ev = {k: [] for k in calls}
    for it in range(warmup + iters):
        for k, fn in calls.items():              # interleaved: all see the same clocks and the same neighbours
            pair = timed(fn)
            if it >= warmup:
                ev[k].append(pair)
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}


def case(label, B, iters, warmup):
    model, data, ctx = make(label)
    x, c = data(B), ctx(B)
    noise = model.context_noise(c)
    latents, _ = model.encode(x, c, noise=noise)
    leaves = [t.clone().requires_grad_(True) for t in latents]
    gx = torch.randn_like(x)

    def decode():
        model.decode(latents, c, noise=noise)

    def decode_grad():
        for t in leaves:
            t.grad = None
        model.decode(leaves, c, noise=noise, differentiable=True).backward(gx)

    def score():
        model.score(x, context=c)

    t = interleaved({"decode": decode, "decode+grad": decode_grad, "score": score}, iters, warmup)
    res = {"model": label, "B": B, "iters": iters, "warmup": warmup}
    for k, v in t.items():
        res[k + " ms"] = round(statistics.median(v), 3)
        res[k + " ms min/max"] = [round(min(v), 3), round(max(v), 3)]
    print(json.dumps(res), flush=True)


def kernels(B, iters, warmup):
    L, P, st = _hip.lib(), _hip.p, _hip.stream()
    model, _, ctx = make("cifar10_onehot_cf")
    c = ctx(B)
    by_width = {}
    for m in model.sequence_modules:
        if type(m) is Coupling:
            by_width.setdefault(m.NN[4].out_channels, m)
    us = lambda v: round(statistics.median(v) * 1e3, 1)
    with torch.no_grad():
        for C, H in ((16, 16), (32, 8), (64, 4)):
            r = lambda *sh: torch.randn(*sh, device=dev)
            m = by_width[C]
            z, g, out = r(B, C, H, H), r(B, C, H, H), torch.empty(B, C, H, H, device=dev)
            x, rec = _coupling_ctx_inverse(m, z, c)
            sbias, mode, ws = rec.sbias, rec.mode, rec.ws
            wsb = m._ctx_step_bwd_tables(mode, C, H, H, dev)
            # the generalist's step on the same conditioner: an orthogonal 1x1 and an ActNorm in front
            Wm, t, logs = torch.linalg.qr(r(C, C).cpu())[0].contiguous().to(dev), 0.1 * r(C), 0.1 * r(C)
            f = lambda v: _hip.f32(v.detach())
            c1, c2, c3 = m.NN[0], m.NN[2], m.NN[4]
            buf = lambda n: torch.empty(n, device=dev, dtype=torch.uint8)
            wsg, wsi = buf(L.cf_flow_step_ws_bytes(C, H, H)), buf(L.cf_flow_step_inv_ws_bytes(C, H, H))
            _hip.call("cf_flow_step_prepare", P(Wm), P(t), P(logs), P(f(c1.weight)), P(f(c1.bias)), P(f(c2.weight)), P(f(c2.bias)),
                      P(f(c3.weight)), P(f(c3.bias)), P(wsg), C, H, H, st)
            _hip.call("cf_flow_step_inv_prepare", P(Wm), P(t), P(logs), P(wsi), C, H, H, st)
            gld = torch.zeros(B, device=dev)
            m1, m2 = 0.1 * r(B, C * C), 0.1 * r(B, 2 * C)
            n = C * H * H
            calls = {
                "cf_flow_step_inv_ctx": lambda: _hip.call("cf_flow_step_inv_ctx", P(z), P(out), P(ws), P(sbias), mode, B, C, H, H, n, st),
                "cf_flow_step_inv": lambda: _hip.call("cf_flow_step_inv", P(z), P(out), P(wsg), P(wsi), B, C, H, H, n, 0, st),
                "walk: one launch + CN": lambda: _coupling_ctx_inverse(m, z, c),
                "walk: Coupling.reverse(z, c)": lambda: m.reverse(z, c),
                "cf_flow_step_inv_bwd_ctx_data": lambda: _hip.call("cf_flow_step_inv_bwd_ctx_data", P(x), P(g), P(ws), P(wsb), P(sbias), mode,
                                                                    P(out), B, C, H, H, n, st),
                "cf_flow_step_bwd_ctx_data": lambda: _hip.call("cf_flow_step_bwd_ctx_data", P(x), P(g), P(gld), P(ws), P(wsb), P(sbias), P(out),
                                                                B, C, H, H, n, st),
                "cf_affine_ctx_inv_bwd_data": lambda: _hip.call("cf_affine_ctx_inv_bwd_data", P(g), P(m1), P(Wm), P(m2), P(logs), P(out), B, C,
                                                                 H, H, 0, st),
                "cf_affine_ctx_inv": lambda: _hip.call("cf_affine_ctx_inv", P(z), P(m1), P(Wm), P(m2), P(t), P(logs), P(out), B, C, H, H, n, 0,
                                                        st),
            }
            tm = interleaved(calls, iters, warmup)
            res = {"level": [C, H, H], "B": B, "bias mode": mode}
            res.update({k + " us": us(v) for k, v in tm.items()})
            print(json.dumps(res), flush=True)
            del z, g, out, x, rec
            torch.cuda.empty_cache()


for cs in [c for c in args.cases.split(",") if c]:
    label, B = cs.split(":")
    case(label, int(B), args.iters, args.warmup)
    torch.cuda.empty_cache()
if args.kernels:
    kernels(args.kernels, args.iters, args.warmup)
