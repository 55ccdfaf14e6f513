#!/usr/bin/env python3
"""Time of `flow.score(x)` (the input gradient of log p(x): data-only walk) next to `log_prob(x)` and to the training forward +
backward (`logp.sum().backward()` with every parameter trainable, no optimizer) - in ONE process, interleaved call by call.

usage: score_bench.py [--cases cifar10:16384,cifar10:256,mnist:16384,smap:32768] [--iters 20] [--warmup 3] [--md] [--affine B]

A case `spec:<dataset>_<enc_emb>[_<enc_type>][_cf]:<B>` (e.g. spec:cifar10_onehot_cf:8192, spec:cifar10_eye:8192) is the
specialist flow `create_model(generalist=False, ...)` with random contexts: `score(x, context=c)`, `log_prob(x, c)` and the
specialist training forward + backward (the parameters that train under that configuration).

Per case one JSON line: medians (and min / max) of HIP-event times per call after the warm-up calls.  --md: a markdown table
behind the JSON lines.  On a tree without `FlowSequential.score` (or without the specialist form of it) the score column is null
and the other two are measured all the same (the training number of two commits is compared with this one script).
--affine B: cf_affine_ctx_bwd_data next to cf_affine_ctx_fwd at the three image levels, B samples, interleaved: time and
achieved bytes/s from 4 (2 C HW + C^2 + C) bytes per sample."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import contextflow_amd as cfa

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="cifar10:16384,cifar10:256,mnist:16384,smap:32768")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--md", action="store_true")
ap.add_argument("--affine", type=int, default=0)
args = ap.parse_args()
dev = "cuda:0"


CONTEXTS = {"mnist": [64], "cifar10": [15, 5], "smap": [55], "atm": [68]}


def make(name, B, spec=None):
    """(model, x, context): spec = the part of a specialist case behind the dataset, e.g. ["onehot", "cf"]; context None for a
    generalist."""
    torch.manual_seed(0)
    cfg, ds, M = cfa.preset_config(name)
    data = (lambda n: torch.rand(n, *ds, device=dev)) if name in ("smap", "atm") else (lambda n: torch.randint(0, 256, (n, *ds), device=dev).float())
    if spec is None:
        model = cfa.create_model(cfg, ds, M).to(dev)
        with torch.no_grad():
            model(data(256))              # ActNorm init
        return model, data(B), None
    cf = spec[-1] == "cf"
    kinds = spec[:-1] if cf else spec
    cfg.update(generalist=False, enc_emb=kinds[0], enc_type=kinds[1] if len(kinds) > 1 else "uniform", contextflow=cf)
    model = cfa.create_model(cfg, ds, M, contexts=CONTEXTS[name]).to(dev)
    ctx = lambda n: torch.stack([torch.randint(0, k, (n,), device=dev) for k in CONTEXTS[name]], dim=1)
    with torch.no_grad():
        model(data(256), ctx(256))        # ActNorm init
    return model, data(B), ctx(B)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def case(label, name, B, iters, warmup, spec=None):
    model, x, ctx = make(name, B, spec)
    params = list(model.parameters())

    def log_prob():
        with torch.no_grad():
            model.log_prob(x, ctx)

    def score():
        model.score(x) if ctx is None else model.score(x, context=ctx)

    def train():
        for p in params:
            p.grad = None
        model.log_prob(x, ctx).sum().backward()

    calls = {"log_prob": log_prob, "train fwd+bwd": train}
    if hasattr(model, "score"):
        try:                                     # (a tree whose score stops at specialist flows: the column stays null)
            score()
            calls["score"] = score
        except (NotImplementedError, TypeError):
            pass
    ev = {k: [] for k in calls}
    for it in range(warmup + iters):
        for k, fn in calls.items():              # interleaved: all three see the same clocks and the same neighbours
            pair = timed(fn)
            if it >= warmup:
                ev[k].append(pair)
    torch.cuda.synchronize()
    res = {"model": label, "B": B, "iters": iters, "warmup": warmup}
    for k in ("score", "log_prob", "train fwd+bwd"):
        if k not in ev:
            res[k + " ms"] = None
            continue
        t = [a.elapsed_time(b) for a, b in ev[k]]
        res[k + " ms"] = round(statistics.median(t), 3)
        res[k + " ms min/max"] = [round(min(t), 3), round(max(t), 3)]
    print(json.dumps(res), flush=True)
    return res


def affine(B, iters, warmup):
    """cf_affine_ctx_bwd_data and cf_affine_ctx_fwd on the same operands at the three image levels, interleaved."""
    from contextflow_amd.layers import _hip
    if not hasattr(_hip.lib(), "cf_affine_ctx_bwd_data"):
        return
    P, st = _hip.p, _hip.stream()
    for C, H, W in ((16, 16, 16), (32, 8, 8), (64, 4, 4)):
        r = lambda *sh: torch.randn(*sh, device=dev)
        x, m1, m2, Wm, t, logs = r(B, C, H, W), 0.1 * r(B, C * C), 0.1 * r(B, 2 * C), r(C, C), r(C), 0.1 * r(C)
        z, ldj, gx = torch.empty_like(x), torch.empty(B, device=dev), torch.empty_like(x)
        calls = {"cf_affine_ctx_fwd": lambda: _hip.call("cf_affine_ctx_fwd", P(x), P(m1), P(Wm), P(m2), P(t), P(logs), None, 0.0, P(z),
                                                        P(ldj), B, C, H, W, C * H * W, 0, 0, 0, st),
                 "cf_affine_ctx_bwd_data": lambda: _hip.call("cf_affine_ctx_bwd_data", P(x), P(m1), P(Wm), P(m2), P(logs), P(gx), B, C, H,
                                                             W, C * H * W, 0, st)}
        ev = {k: [] for k in calls}
        for it in range(warmup + iters):
            for k, fn in calls.items():
                pair = timed(fn)
                if it >= warmup:
                    ev[k].append(pair)
        torch.cuda.synchronize()
        nbytes = 4 * (2 * C * H * W + C * C + C) * B
        res = {"affine": [C, H, W], "B": B}
        for k in calls:
            us = statistics.median(a.elapsed_time(b) for a, b in ev[k]) * 1e3
            res[k + " us"] = round(us, 2)
            res[k + " GB/s"] = round(nbytes / us * 1e-3, 1)
        print(json.dumps(res), flush=True)


rows = []
for c in [c for c in args.cases.split(",") if c]:
    parts = c.split(":")
    if parts[0] == "spec":
        kinds = parts[1].split("_")
        rows.append(case(parts[1], kinds[0], int(parts[2]), args.iters, args.warmup, kinds[1:]))
    else:
        rows.append(case(parts[0], parts[0], int(parts[1]), args.iters, args.warmup))
    torch.cuda.empty_cache()
if args.affine:
    affine(args.affine, args.iters, args.warmup)
if args.md:
    f = lambda r, k: "-" if r[k + " ms"] is None else "%.3f (%.3f - %.3f)" % ((r[k + " ms"],) + tuple(r[k + " ms min/max"]))
    print("| model | B | score ms | log_prob ms | train fwd+bwd ms |")
    print("|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %s | %s | %s |" % (r["model"], r["B"], f(r, "score"), f(r, "log_prob"), f(r, "train fwd+bwd")))
