#!/usr/bin/env python3
"""Sampling throughput (`flow.sample`: prior draw + fused inverse steps).

usage: sample_bench.py [name] [B] [iters] [--labels L] [--temperature T]
       sample_bench.py --compare [--names cifar10,mnist] [B] [--iters 20] [--warmup 5]
       sample_bench.py --logp [--iters 20] [--warmup 5]

--labels L: an integer class for every sample, or `cycle` (sample i gets class i % M); --temperature T: scale factor of the prior
draws.  Either one selects the one-launch-per-level draw (cf_gmm_draw) instead of the reference's multinomial / randn / gather /
concatenate.
--compare: in ONE process, for each model, `sample(B)` against `sample(B, labels=1)` - the same class-mixture - as medians
of HIP-event times per call after the warm-up calls, interleaved call by call, and per prior level the time of the cf_gmm_draw
launch alone with the bytes it moves (write 4 B (D1 + D), read 4 B D1).  One JSON line per model.
--logp: in ONE process, cifar10 and mnist at 16 384 samples and smap at 32 768: `sample(B)`, `sample(B, return_logp=True)` and
`sample(B)` followed by `log_prob(x)`, interleaved, and the inverse-step launches of both walks per level.  One JSON line per model."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import contextflow_amd as cfa

ap = argparse.ArgumentParser()
ap.add_argument("name", nargs="?", default="cifar10")
ap.add_argument("B", nargs="?", type=int, default=16384)
ap.add_argument("iters_pos", nargs="?", type=int, default=None)
ap.add_argument("--iters", type=int, default=None)
ap.add_argument("--warmup", type=int, default=None)
ap.add_argument("--labels", default=None)
ap.add_argument("--temperature", type=float, default=1.0)
ap.add_argument("--compare", action="store_true")
ap.add_argument("--names", default="cifar10,mnist")
ap.add_argument("--logp", action="store_true")
args = ap.parse_args()
dev = "cuda:0"


def make(name):
    torch.manual_seed(0)
    cfg, ds, M = cfa.preset_config(name)
    model = cfa.create_model(cfg, ds, M).to(dev)
    x = torch.randint(0, 256, (256, *ds), device=dev).float()
    with torch.no_grad():
        model(x)                      # ActNorm init
    return model, M


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    return e0, e1, out


def compare(name, B, iters, warmup):
    model, M = make(name)
    calls = {"default": lambda: model.sample(B), "labels=1": lambda: model.sample(B, labels=1)}
    ev = {k: [] for k in calls}
    with torch.no_grad():
        for it in range(warmup + iters):
            for k, fn in calls.items():          # interleaved: both see the same clocks and the same neighbours
                e0, e1, s = timed(fn)
                if it >= warmup:
                    ev[k].append((e0, e1))
        torch.cuda.synchronize()
        res = {"model": name, "B": B, "iters": iters, "warmup": warmup}
        for k, pairs in ev.items():
            t = [a.elapsed_time(b) for a, b in pairs]
            res[k + " ms"] = round(statistics.median(t), 4)
            res[k + " ms min/max"] = [round(min(t), 4), round(max(t), 4)]
        # the draw launch of every level alone, in the order `sample` meets them: the prior, then the SplitPriors from the last
        splits = [m for m in model.sequence_modules if isinstance(m, cfa.layers.SplitPrior)]
        levels = []
        for dist, kept in [(model.dist, False)] + [(m.dist, True) for m in reversed(splits)]:
            C, H, W = dist.mG.shape[2:]
            z1 = torch.randn(B, C, H, W, device=dev) if kept else None
            D, D1 = C * H * W, (C * H * W if kept else 0)
            t = []
            for it in range(warmup + iters):
                e0, e1, _ = timed(lambda: dist.draw(B, 1, 1.0, z1=z1))
                if it >= warmup:
                    t.append((e0, e1))
            torch.cuda.synchronize()
            us = statistics.median(a.elapsed_time(b) for a, b in t) * 1e3
            nbytes = 4 * B * (D1 + D) + 4 * B * D1
            levels.append({"D": D, "D1": D1, "us": round(us, 2), "GB/s": round(nbytes / us * 1e-3, 1)})
        res["cf_gmm_draw levels (incl. the nonce draw and the output allocation)"] = levels
    print(json.dumps(res))


def logp_bench(name, B, iters, warmup):
    """`sample(B)`, `sample(B, return_logp=True)` and `sample(B)` followed by `log_prob(x)` - what the density of a draw cost before
    the flag - interleaved call by call, medians of HIP-event times; then, per resolution level, the inverse-step launches of
    the plain and of the flagged walk (cf_flow_step_inv / cf_flow_step_inv_ld), from the events around each launch."""
    model, M = make(name)

    def two_pass():
        x = model.sample(B)
        return model.log_prob(x)
    calls = {"sample": lambda: model.sample(B), "sample+logp": lambda: model.sample(B, return_logp=True), "sample; log_prob": two_pass}
    ev = {k: [] for k in calls}
    with torch.no_grad():
        for it in range(warmup + iters):
            for k, fn in calls.items():
                e0, e1, _ = timed(fn)
                if it >= warmup:
                    ev[k].append((e0, e1))
        torch.cuda.synchronize()
        res = {"model": name, "B": B, "iters": iters, "warmup": warmup}
        for k, pairs in ev.items():
            t = [a.elapsed_time(b) for a, b in pairs]
            res[k + " ms"] = round(statistics.median(t), 4)
            res[k + " ms min/max"] = [round(min(t), 4), round(max(t), 4)]
        levels = {}
        for it in range(2 + iters):
            for k, flag in (("inv", False), ("inv_ld", True)):
                model.inv_events = []
                model.sample(B, return_logp=flag)
                torch.cuda.synchronize()
                if it >= 2:
                    for e0, e1, _, C, HW in model.inv_events:
                        levels.setdefault((C, HW), {"inv": [], "inv_ld": []})[k].append(e0.elapsed_time(e1))
                model.inv_events = None
        res["inverse-step launches, us (median per launch)"] = [
            {"C": C, "HW": HW, "launches per call": len(v["inv"]) // iters, "cf_flow_step_inv": round(statistics.median(v["inv"]) * 1e3, 1),
             "cf_flow_step_inv_ld": round(statistics.median(v["inv_ld"]) * 1e3, 1)} for (C, HW), v in sorted(levels.items())]
    print(json.dumps(res))


if args.logp:
    for nm, B in (("cifar10", 16384), ("mnist", 16384), ("smap", 32768)):
        logp_bench(nm, B, args.iters or 20, 5 if args.warmup is None else args.warmup)
    sys.exit(0)

if args.compare:
    for nm in args.names.split(","):
        compare(nm, args.B, args.iters or 20, 5 if args.warmup is None else args.warmup)
    sys.exit(0)

name, B = args.name, args.B
iters = args.iters or args.iters_pos or 10
model, M = make(name)
kw = {}
if args.labels is not None:
    kw["labels"] = torch.arange(B, device=dev) % M if args.labels == "cycle" else int(args.labels)
if args.temperature != 1.0:
    kw["temperature"] = args.temperature
with torch.no_grad():
    for _ in range(3 if args.warmup is None else args.warmup):
        s = model.sample(B, **kw)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters):
        s = model.sample(B, **kw)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / iters
print("%s sample B=%d%s: %.2f ms = %.0f samples/s (finite %s)" % (name, B, "".join(" %s=%s" % (k, args.labels if k == "labels" else v) for k, v in kw.items()),
                                                                 dt * 1e3, B / dt, torch.isfinite(s).all().item()))
