#!/usr/bin/env python3
"""Sampling from the specialist (context-conditioned) flows: `sample(B, context)` next to `log_prob(x, context)` of the same flow
and next to the generalist `sample(B)` of the same dataset.

usage: specialist_sample_bench.py [--cases cifar10_onehot_cf:8192,cifar10_eye:8192,mnist_eye_cf:8192] [--iters 20] [--warmup 5]
                                  [--affine B] [--launches cifar10_onehot_cf:256]

One JSON line per case: medians (min / max) of HIP-event times per call after the warm-up calls, the three calls interleaved
call by call in ONE process (same clocks, same neighbours).  A tree without the specialist inverse prints null for it.
--affine B: cf_affine_ctx_inv next to cf_affine_ctx_fwd on the same operands at the three image levels, B samples, interleaved:
time and the bytes both move (x, z, m1, m2).
--launches case:B: the entry points one `sample(B, context)` call passes to _hip.call, in order, with their counts."""
import argparse, collections, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import contextflow_amd as cfa
from contextflow_amd.layers import _hip

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="cifar10_onehot_cf:8192,cifar10_eye:8192,mnist_eye_cf:8192")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--affine", type=int, default=0)
ap.add_argument("--launches", default="")
args = ap.parse_args()
dev = "cuda:0"
CONTEXTS = {"mnist": [64], "cifar10": [15, 5]}


def make(name, spec=None):
    """(model, data(n), context(n) | None): spec = the part of a specialist case behind the dataset, e.g. ["onehot", "cf"]."""
    torch.manual_seed(0)
    cfg, ds, M = cfa.preset_config(name)
    data = lambda n: torch.randint(0, 256, (n, *ds), device=dev).float()
    if spec is None:
        model = cfa.create_model(cfg, ds, M).to(dev)
        with torch.no_grad():
            model(data(256))              # ActNorm init
        return model, data, None
    cf = spec[-1] == "cf"
    kinds = spec[:-1] if cf else spec
    cfg.update(generalist=False, enc_emb=kinds[0], enc_type=kinds[1] if len(kinds) > 1 else "uniform", contextflow=cf)
    model = cfa.create_model(cfg, ds, M, contexts=CONTEXTS[name]).to(dev)
    ctx = lambda n: torch.stack([torch.randint(0, k, (n,), device=dev) for k in CONTEXTS[name]], dim=1)
    with torch.no_grad():
        model(data(256), ctx(256))        # ActNorm init
    return model, data, ctx


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def interleaved(calls, iters, warmup):
    ev = {k: [] for k in calls}
    with torch.no_grad():
        for it in range(warmup + iters):
            for k, fn in calls.items():
                pair = timed(fn)
                if it >= warmup:
                    ev[k].append(pair)
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}


def case(label, B, iters, warmup):
    kinds = label.split("_")
    spec, data, ctx = make(kinds[0], kinds[1:])
    gen, _, _ = make(kinds[0])
    x, c = data(B), ctx(B)
    calls = {"log_prob(x, context)": lambda: spec.log_prob(x, c), "generalist sample(B)": lambda: gen.sample(B)}
    try:
        spec.sample(B, c)
        calls["sample(B, context)"] = lambda: spec.sample(B, c)
    except (NotImplementedError, TypeError):
        pass
    t = interleaved(calls, iters, warmup)
    res = {"model": label, "B": B, "iters": iters, "warmup": warmup}
    for k in ("sample(B, context)", "log_prob(x, context)", "generalist sample(B)"):
        res[k + " ms"] = round(statistics.median(t[k]), 3) if k in t else None
        if k in t:
            res[k + " ms min/max"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
    print(json.dumps(res), flush=True)


def affine(B, iters, warmup):
    if not hasattr(_hip.lib(), "cf_affine_ctx_inv"):
        return
    P, st = _hip.p, _hip.stream()
    for C, H, W in ((16, 16, 16), (32, 8, 8), (64, 4, 4)):
        r = lambda *sh: torch.randn(*sh, device=dev)
        x, m1, m2, t, logs = r(B, C, H, W), 0.1 * r(B, C * C), 0.1 * r(B, 2 * C), r(C), 0.1 * r(C)
        Wm = torch.linalg.qr(r(C, C).cpu())[0].contiguous().to(dev)
        z, ldj, back = torch.empty_like(x), torch.empty(B, device=dev), torch.empty_like(x)
        calls = {"cf_affine_ctx_fwd": lambda: _hip.call("cf_affine_ctx_fwd", P(x), P(m1), P(Wm), P(m2), P(t), P(logs), None, 0.0, P(z),
                                                        P(ldj), B, C, H, W, C * H * W, 0, 0, 0, st),
                 "cf_affine_ctx_inv": lambda: _hip.call("cf_affine_ctx_inv", P(z), P(m1), P(Wm), P(m2), P(t), P(logs), P(back), B, C, H, W,
                                                        C * H * W, 0, st)}
        tt = interleaved(calls, iters, warmup)
        nbytes = 4 * (2 * C * H * W + C * C + 2 * C) * B
        res = {"affine": [C, H, W], "B": B, "round trip max|x - back|": round(float((x - back).abs().max()), 8)}
        for k in calls:
            us = statistics.median(tt[k]) * 1e3
            res[k + " us"] = round(us, 2)
            res[k + " GB/s"] = round(nbytes / us * 1e-3, 1)
        print(json.dumps(res), flush=True)


def launches(label, B):
    kinds = label.split("_")
    spec, _, ctx = make(kinds[0], kinds[1:])
    c = ctx(B)
    names, real = [], _hip.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    _hip.call = recording
    try:
        with torch.no_grad():
            spec.sample(B, c)
    finally:
        _hip.call = real
    torch.cuda.synchronize()
    print(json.dumps({"model": label, "B": B, "launches of one sample(B, context)": len(names),
                      "by entry point": dict(collections.Counter(names).most_common())}), flush=True)


for cs in [c for c in args.cases.split(",") if c]:
    label, B = cs.split(":")
    case(label, int(B), args.iters, args.warmup)
    torch.cuda.empty_cache()
if args.affine:
    affine(args.affine, args.iters, args.warmup)
if args.launches:
    label, B = args.launches.split(":")
    launches(label, int(B))
