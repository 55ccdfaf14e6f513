#!/usr/bin/env python3
"""Time of `decode(latents, differentiable=True)` + backward (the latent gradient of the backward walk) next to `decode` alone and
to `score(x)` - in ONE process, interleaved call by call - and of the inverse step's VJP kernel per level next to
cf_flow_step_bwd_ctx_data on the same shapes.

usage: decode_grad_bench.py [--cases cifar10:256,cifar10:16384,mnist:256,mnist:16384] [--iters 20] [--warmup 5] [--kernels B] [--md]

Per case one JSON line: medians (and min / max) of HIP-event times per call after the warm-up calls.  --kernels B: the two
kernels at the four levels of the backward dispatch, B samples, interleaved.  --md: markdown tables behind the JSON lines."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import contextflow_amd as cfa

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="cifar10:256,cifar10:16384,mnist:256,mnist:16384")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--kernels", type=int, default=0)
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


def case(name, B, iters, warmup):
    torch.manual_seed(0)
    cfg, ds, M = cfa.preset_config(name)
    model = cfa.create_model(cfg, ds, M).to(dev)
    data = lambda n: torch.randint(0, 256, (n, *ds), device=dev).float()
    with torch.no_grad():
        model(data(256))                         # ActNorm init
    x = data(B)
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
    res = {"model": name, "B": B, "iters": iters, "warmup": warmup}
    for k, v in t.items():
        res[k + " ms"] = round(statistics.median(v), 3)
        res[k + " ms min/max"] = [round(min(v), 3), round(max(v), 3)]
    print(json.dumps(res), flush=True)
    return res


def kernels(B, iters, warmup):
    """cf_flow_step_inv_bwd_data and cf_flow_step_bwd_ctx_data (the same recompute, its own epilogue and one more / one less 1x1
    phase) on the same operands at the four levels."""
    from contextflow_amd.layers import _hip
    L, P, st = _hip.lib(), _hip.p, _hip.stream()
    rows = []
    for C, H in ((8, 16), (16, 16), (32, 8), (64, 4)):
        r = lambda *sh: torch.randn(*sh, device=dev)
        Wm = torch.linalg.qr(r(C, C))[0].contiguous()
        t, logs = 0.1 * r(C), 0.1 * r(C)
        w1, b1, w2, b2, w3, b3 = 0.2 * r(2 * C, C // 2, 1, 1), 0.1 * r(2 * C), 0.05 * r(2 * C, 2 * C, 3, 3), 0.1 * r(2 * C), 0.05 * r(C, 2 * C, 1, 1), 0.1 * r(C)
        buf = lambda n: torch.empty(n, device=dev, dtype=torch.uint8)
        ws, wsb = buf(L.cf_flow_step_ws_bytes(C, H, H)), buf(L.cf_flow_step_bwd_ws_bytes(C, H, H))
        wsi, wsv = buf(L.cf_flow_step_inv_ws_bytes(C, H, H)), buf(L.cf_flow_step_inv_bwd_ws_bytes(C, H, H))
        _hip.call("cf_flow_step_prepare", P(Wm), P(t), P(logs), P(w1), P(b1), P(w2), P(b2), P(w3), P(b3), P(ws), C, H, H, st)
        _hip.call("cf_flow_step_bwd_prepare", P(Wm), P(logs), P(w1), P(w2), P(w3), P(wsb), C, H, H, st)
        _hip.call("cf_flow_step_inv_prepare", P(Wm), P(t), P(logs), P(wsi), C, H, H, st)
        _hip.call("cf_flow_step_inv_bwd_prepare", P(wsi), P(logs), P(wsv), C, H, H, st)
        x, g, gld, sb, out = r(B, C, H, H), r(B, C, H, H), r(B), torch.zeros(B, C, device=dev), torch.empty(B, C, H, H, device=dev)
        calls = {"cf_flow_step_inv_bwd_data": lambda: _hip.call("cf_flow_step_inv_bwd_data", P(x), P(g), P(ws), P(wsb), P(wsv), P(out), B, C, H, H,
                                                                C * H * H, st),
                 "cf_flow_step_bwd_ctx_data": lambda: _hip.call("cf_flow_step_bwd_ctx_data", P(x), P(g), P(gld), P(ws), P(wsb), P(sb), P(out), B, C,
                                                                H, H, C * H * H, st)}
        tm = interleaved(calls, iters, warmup)
        res = {"level": [C, H, H], "B": B}
        for k, v in tm.items():
            res[k + " us"] = round(statistics.median(v) * 1e3, 1)
        print(json.dumps(res), flush=True)
        rows.append(res)
    return rows


rows = []
for c in [c for c in args.cases.split(",") if c]:
    name, B = c.split(":")
    rows.append(case(name, int(B), args.iters, args.warmup))
    torch.cuda.empty_cache()
krows = kernels(args.kernels, args.iters, args.warmup) if args.kernels else []
if args.md:
    f = lambda r, k: "%.3f (%.3f - %.3f)" % ((r[k + " ms"],) + tuple(r[k + " ms min/max"]))
    print("| model | B | decode ms | decode(differentiable) + backward ms | score ms |")
    print("|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %s | %s | %s |" % (r["model"], r["B"], f(r, "decode"), f(r, "decode+grad"), f(r, "score")))
    if krows:
        print("| level | B | cf_flow_step_inv_bwd_data us | cf_flow_step_bwd_ctx_data us |")
        print("|---|---|---|---|")
        for r in krows:
            print("| %s | %d | %.1f | %.1f |" % (tuple(r["level"]), r["B"], r["cf_flow_step_inv_bwd_data us"], r["cf_flow_step_bwd_ctx_data us"]))
