#!/usr/bin/env python3
"""Time of `decode(latents, differentiable=True)` + backward on the transformer flows (the latent gradient of their backward walk)
next to `decode` alone and to `score(x)` - in ONE process, interleaved call by call - and of the inverse transformer step's VJP
kernel next to cf_vit_step_bwd (the training backward: the same recompute and walk, plus the operand planes) on the same operands.

usage: vit_decode_grad_bench.py [--cases smap:256,smap:32768] [--iters 20] [--warmup 5] [--kernels B] [--sample N] [--md]

Per case one JSON line: medians (and min / max) of HIP-event times per call after the warm-up calls.  --kernels B: the two
kernels at B samples, interleaved.  --sample N: `sample(N)` alone (an existing path: for a comparison between two commits).
--md: markdown tables behind the JSON lines."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import contextflow_amd as cfa

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="smap:256,smap:32768")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--kernels", type=int, default=0)
ap.add_argument("--sample", type=int, default=0)
ap.add_argument("--md", action="store_true")
args = ap.parse_args()
dev = "cuda:0"


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


def summary(res, t, unit="ms", scale=1.0):
    for k, v in t.items():
        res["%s %s" % (k, unit)] = round(statistics.median(v) * scale, 3)
        res["%s %s min/max" % (k, unit)] = [round(min(v) * scale, 3), round(max(v) * scale, 3)]
    print(json.dumps(res), flush=True)
    return res


def build(name):
    torch.manual_seed(0)
    cfg, ds, M = cfa.preset_config(name)
    model = cfa.create_model(cfg, ds, M).to(dev)
    with torch.no_grad():
        model(torch.randn(256, *ds, device=dev))     # ActNorm init
    return model, ds


def case(name, B, iters, warmup):
    model, ds = build(name)
    x = torch.randn(B, *ds, device=dev)
    latents, _ = model.encode(x)
    leaves = [t.clone().requires_grad_(True) for t in latents]
    gx = torch.randn(B, *ds, device=dev)

    def decode():
        model.decode(latents)

    def decode_grad():
        for t in leaves:
            t.grad = None
        model.decode(leaves, differentiable=True).backward(gx)

    def score():
        model.score(x)

    t = interleaved({"decode": decode, "decode+grad": decode_grad, "score": score}, iters, warmup)
    return summary({"model": name, "B": B, "iters": iters, "warmup": warmup}, t)


def sample(name, N, iters, warmup):
    model, _ = build(name)
    t = interleaved({"sample": lambda: model.sample(N)}, iters, warmup)
    return summary({"model": name, "sample": N, "iters": iters, "warmup": warmup}, t)


def kernels(B, iters, warmup):
    """cf_vit_inv_step_bwd_data and cf_vit_step_bwd (recompute form, no tape) on the same x, upstream and tables, depth 6."""
    from contextflow_amd.layers import _hip
    L, P, st = _hip.lib(), _hip.p, _hip.stream()
    C, HW, depth = 26, 8, 6
    torch.manual_seed(0)
    conv, act, cpl = cfa.layers.Conv1x1((C, HW, 1)).to(dev), cfa.layers.ActNorm((C, HW, 1)).to(dev), cfa.layers.TransCoupling((C, HW, 1), (2, 1)).to(dev)
    with torch.no_grad():
        act.NN_t.normal_(0, 0.1); act.NN_logs.normal_(0, 0.1)
    t = cfa.layers.TransCoupling.step_tables([(cpl, conv.NN, act.NN_t, act.NN_logs)], torch.device(dev), "rs", winv=True, bwd=True)[0]
    wsv = torch.empty(L.cf_vit_inv_step_bwd_ws_bytes(C), device=dev, dtype=torch.uint8)
    _hip.call("cf_vit_inv_step_bwd_prepare", P(t.winv), P(_hip.f32(act.NN_logs.detach())), P(wsv), C, st)
    r = lambda *sh: torch.randn(*sh, device=dev)
    x, g, gld, out = r(B, C, HW, 1), r(B, C, HW, 1), r(B), torch.empty(B, C, HW, 1, device=dev)
    planes = torch.empty(L.cf_vit_step_bwd_plane_floats(B, C, depth), device=dev)
    lnp = torch.empty(L.cf_vit_step_bwd_ln_floats(B, C, depth), device=dev)
    calls = {"cf_vit_inv_step_bwd_data": lambda: _hip.call("cf_vit_inv_step_bwd_data", P(x), P(g), P(t.ws), P(t.wsb), P(wsv), P(out), B, C, depth,
                                                           C * HW, st),
             "cf_vit_step_bwd": lambda: _hip.call("cf_vit_step_bwd", P(x), P(g), P(gld), P(out), P(t.ws), P(t.wsb), P(planes), P(lnp), None, B, C,
                                                  depth, C * HW, st)}
    return summary({"B": B, "depth": depth}, interleaved(calls, iters, warmup), "us", 1e3)


rows = []
for c in [c for c in args.cases.split(",") if c]:
    name, B = c.split(":")
    rows.append(case(name, int(B), args.iters, args.warmup))
    torch.cuda.empty_cache()
krow = kernels(args.kernels, args.iters, args.warmup) if args.kernels else None
if args.sample:
    sample("smap", args.sample, args.iters, args.warmup)
if args.md:
    f = lambda r, k, u="ms": "%.3f (%.3f - %.3f)" % ((r["%s %s" % (k, u)],) + tuple(r["%s %s min/max" % (k, u)]))
    print("| model | B | decode ms | decode(differentiable) + backward ms | score ms |")
    print("|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %s | %s | %s |" % (r["model"], r["B"], f(r, "decode"), f(r, "decode+grad"), f(r, "score")))
    if krow:
        print("| B | cf_vit_inv_step_bwd_data us | cf_vit_step_bwd us |")
        print("|---|---|---|")
        print("| %d | %s | %s |" % (krow["B"], f(krow, "cf_vit_inv_step_bwd_data", "us"), f(krow, "cf_vit_step_bwd", "us")))
