#!/usr/bin/env python3
"""Time of the spline-coupling kernels - cf_spline_coupling forward and inverse, cf_spline_coupling_bwd - next to
cf_coupling_apply, the affine twin, on the same shapes, interleaved call by call.

usage: spline_coupling_bench.py [--shapes 16x16x16,32x8x8,64x4x4] [--batch 16384] [--bins 8] [--iters 20] [--warmup 5]
                                [--limit 240] [--md]

Every shape is measured by a child process of its own under a time limit of --limit seconds; a child that fails or runs out of
time ends the run.  Per shape one JSON line: medians of HIP-event times per call after the warm-up calls, in us, and the
achieved bytes/s from the bytes the kernels must move per sample:
    spline forward / inverse   4 (2 C + D (3K-1)) HW        (x, z and the raw knot parameters)
    spline backward            4 (D + 2 C + 2 D (3K-1)) HW  (x1, gz, gx, the parameters and their gradient)
    affine forward             4 (3 C) HW                   (x, z and h = [t | raw])
The inputs: h ~ randn, x1 ~ 2 randn scaled so that a tenth lies outside the tails.  --md: a markdown table behind the JSON lines."""
import argparse, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="16x16x16,32x8x8,64x4x4")
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--bins", type=int, default=8)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--limit", type=int, default=240)
ap.add_argument("--md", action="store_true")
ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
args = ap.parse_args()
TB = 3.0


def one(C, H, W):
    import torch
    from contextflow_amd.layers import _hip
    dev, B, K = "cuda:0", args.batch, args.bins
    D, HW = C // 2, H * W
    nj = 3 * K - 1
    torch.manual_seed(0)
    P, st = _hip.p, _hip.stream()
    x = torch.randn(B, C, H, W, device=dev)
    x1 = 2.0 * torch.randn(B, D, H, W, device=dev)
    x[:, D:] = x1 * (TB / x1.abs().flatten()[: 1 << 20].quantile(0.9))
    h = torch.randn(B, D * nj, H, W, device=dev)
    ha = torch.randn(B, C, H, W, device=dev)
    gz, gld = torch.randn(B, C, H, W, device=dev), torch.randn(B, device=dev)
    z, ldj, gx, gh = torch.empty_like(x), torch.empty(B, device=dev), torch.empty_like(x), torch.empty_like(h)
    bs = C * HW
    calls = {
        "spline fwd": (lambda: _hip.call("cf_spline_coupling", P(x), P(h), P(z), P(ldj), B, C, HW, K, TB, bs, 0, st), 4 * (2 * C + D * nj) * HW),
        "spline inv": (lambda: _hip.call("cf_spline_coupling", P(x), P(h), P(z), P(ldj), B, C, HW, K, TB, bs, 1, st), 4 * (2 * C + D * nj) * HW),
        "spline bwd": (lambda: _hip.call("cf_spline_coupling_bwd", P(x), P(h), P(gz), P(gld), P(gx), P(gh), B, C, HW, K, TB, bs, bs, st),
                       4 * (D + 2 * C + 2 * D * nj) * HW),
        "affine fwd": (lambda: _hip.call("cf_coupling_apply", P(x), P(ha), P(z), P(ldj), B, C, HW, 0, st), 4 * 3 * C * HW),
    }
    ev = {k: [] for k in calls}
    for it in range(args.warmup + args.iters):
        for k, (fn, _) in calls.items():          # interleaved: every kernel sees the same clocks and the same neighbours
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            if it >= args.warmup:
                ev[k].append((e0, e1))
    torch.cuda.synchronize()
    res = {"shape": [C, H, W], "B": B, "K": K, "iters": args.iters, "warmup": args.warmup}
    for k, (_, nbytes) in calls.items():
        t = [a.elapsed_time(b) * 1e3 for a, b in ev[k]]
        us = statistics.median(t)
        res[k + " us"] = round(us, 1)
        res[k + " us min/max"] = [round(min(t), 1), round(max(t), 1)]
        res[k + " TB/s"] = round(nbytes * B / us * 1e-6, 3)
    print(json.dumps(res), flush=True)


if args.one:
    one(*[int(v) for v in args.one.split("x")])
    sys.exit(0)

rows = []
for shape in [s for s in args.shapes.split(",") if s]:
    cmd = [sys.executable, os.path.abspath(__file__), "--one", shape, "--batch", str(args.batch), "--bins", str(args.bins),
           "--iters", str(args.iters), "--warmup", str(args.warmup)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        sys.exit("spline_coupling_bench: %s ran past %d s; nothing more is started" % (shape, args.limit))
    if r.returncode != 0:
        sys.exit("spline_coupling_bench: %s failed with status %d; nothing more is started\n%s" % (shape, r.returncode, r.stderr[-2000:]))
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    rows.append(json.loads(line))
if args.md:
    kinds = ("spline fwd", "spline inv", "spline bwd", "affine fwd")
    print("| shape | B | K | " + " | ".join("%s us (TB/s)" % k for k in kinds) + " |")
    print("|---|---|---|" + "---|" * len(kinds))
    for r in rows:
        print("| %s | %d | %d | " % ("x".join(map(str, r["shape"])), r["B"], r["K"])
              + " | ".join("%.1f (%.2f)" % (r[k + " us"], r[k + " TB/s"]) for k in kinds) + " |")
