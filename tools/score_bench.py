#!/usr/bin/env python3
"""Time of `flow.score(x)` (the input gradient of log p(x): data-only walk) next to `log_prob(x)` and to the training forward +
backward (`logp.sum().backward()` with every parameter trainable, no optimizer) - in ONE process, interleaved call by call.

usage: score_bench.py [--cases cifar10:16384,cifar10:256,mnist:16384,smap:32768] [--iters 20] [--warmup 3] [--md]

Per case one JSON line: medians (and min / max) of HIP-event times per call after the warm-up calls.  --md: a markdown table
behind the JSON lines.  On a tree without `FlowSequential.score` the score column is null and the other two are measured all
the same (the training number of two commits is compared with this one script)."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import contextflow_amd as cfa

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="cifar10:16384,cifar10:256,mnist:16384,smap:32768")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--md", action="store_true")
args = ap.parse_args()
dev = "cuda:0"


def make(name, B):
    torch.manual_seed(0)
    cfg, ds, M = cfa.preset_config(name)
    model = cfa.create_model(cfg, ds, M).to(dev)
    data = (lambda n: torch.rand(n, *ds, device=dev)) if name in ("smap", "atm") else (lambda n: torch.randint(0, 256, (n, *ds), device=dev).float())
    with torch.no_grad():
        model(data(256))              # ActNorm init
    return model, data(B)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def case(name, B, iters, warmup):
    model, x = make(name, B)
    params = list(model.parameters())

    def log_prob():
        with torch.no_grad():
            model.log_prob(x)

    def score():
        model.score(x)

    def train():
        for p in params:
            p.grad = None
        model.log_prob(x).sum().backward()

    calls = {"log_prob": log_prob, "train fwd+bwd": train}
    if hasattr(model, "score"):
        calls["score"] = score
    ev = {k: [] for k in calls}
    for it in range(warmup + iters):
        for k, fn in calls.items():              # interleaved: all three see the same clocks and the same neighbours
            pair = timed(fn)
            if it >= warmup:
                ev[k].append(pair)
    torch.cuda.synchronize()
    res = {"model": name, "B": B, "iters": iters, "warmup": warmup}
    for k in ("score", "log_prob", "train fwd+bwd"):
        if k not in ev:
            res[k + " ms"] = None
            continue
        t = [a.elapsed_time(b) for a, b in ev[k]]
        res[k + " ms"] = round(statistics.median(t), 3)
        res[k + " ms min/max"] = [round(min(t), 3), round(max(t), 3)]
    print(json.dumps(res), flush=True)
    return res


rows = []
for c in args.cases.split(","):
    nm, b = c.split(":")
    rows.append(case(nm, int(b), args.iters, args.warmup))
    torch.cuda.empty_cache()
if args.md:
    f = lambda r, k: "-" if r[k + " ms"] is None else "%.3f (%.3f - %.3f)" % ((r[k + " ms"],) + tuple(r[k + " ms min/max"]))
    print("| model | B | score ms | log_prob ms | train fwd+bwd ms |")
    print("|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %s | %s | %s |" % (r["model"], r["B"], f(r, "score"), f(r, "log_prob"), f(r, "train fwd+bwd")))
