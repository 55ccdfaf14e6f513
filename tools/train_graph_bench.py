#!/usr/bin/env python3
"""Whole training step (forward + hand-written backward + AdamW) captured into ONE HIP graph with torch.cuda.graphs
(launch-bound regimes: the SMAP transformer flow runs ~1800 small kernels per step).  usage: [name] [B] [iters] [clip]
CF_OWN_ADAMW=1: contextflow_amd.optim.FusedAdamW.  A fourth argument `clip`: the reference's loop with warm-up and grad_clip_norm -
FusedAdamW(max_grad_norm=CF_MAX_GRAD_NORM, default 100) and a new param_group['lr'] + push_hyperparameters() before EVERY replay.
`clip` always uses FusedAdamW (torch's AdamW has neither): CF_OWN_ADAMW is not consulted then, and CF_OWN_ADAMW=0 with it is refused.
The replay time is the median of five timed blocks of `iters` replays behind `iters` untimed ones.  Earlier revisions of this
tool timed ONE block without a replay warm-up: to compare a revision with an older one, run THIS file against both trees (it
needs nothing the older package lacks unless `clip` is given), in one session, alternating."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import contextflow_amd as cfa

name = sys.argv[1] if len(sys.argv) > 1 else "smap"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 10
dev = "cuda:0"
torch.manual_seed(0)
cfg, ds, M = cfa.preset_config(name)
model = cfa.create_model(cfg, ds, M).to(dev)
x = torch.rand(B, *ds, device=dev) if M == 1 else torch.randint(0, 256, (B, *ds), device=dev).float()
gt = torch.randint(0, M, (B,), device=dev)
with torch.no_grad():
    model(x[:256])
clip = len(sys.argv) > 4 and sys.argv[4] == "clip"
if clip and os.environ.get("CF_OWN_ADAMW", "1") != "1":
    sys.exit("train_graph_bench: `clip` needs FusedAdamW (CF_OWN_ADAMW=%s given)" % os.environ["CF_OWN_ADAMW"])
opt = (cfa.optim.FusedAdamW(model.parameters(), lr=1e-4, max_grad_norm=float(os.environ.get("CF_MAX_GRAD_NORM", "100"))) if clip
       else cfa.optim.FusedAdamW(model.parameters(), lr=1e-4) if os.environ.get("CF_OWN_ADAMW") == "1"      # CF_OWN_ADAMW=1: contextflow_amd.optim
       else torch.optim.AdamW(model.parameters(), lr=1e-4, capturable=True, fused=True))      # one multi-tensor kernel per step
dim_inv = 1.0 / (ds[0] * ds[1] * ds[2])


def step():
    opt.zero_grad(set_to_none=True)       # the engine takes the buffers the backward returns: no fill / accumulate launches
    logp = dim_inv * model.log_prob(x)
    loss = -logp.mean() if M == 1 else torch.nn.functional.cross_entropy(logp, gt)
    loss.backward()
    opt.step()
    return loss


s = torch.cuda.Stream()
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(s):
    for _ in range(3):
        step()
torch.cuda.current_stream().wait_stream(s)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(iters):
    step()
torch.cuda.synchronize()
eager = (time.perf_counter() - t0) / iters
push = getattr(opt, "push_hyperparameters", None)
if push is not None:
    push()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    loss = step()
torch.cuda.synchronize()
l0 = float(loss)
updates = [0]


def replay():
    if clip:                     # a schedule that moves every step: one scalar fill in front of the replay
        updates[0] += 1
        for group in opt.param_groups:
            group["lr"] = 1e-4 * (1.0 + (updates[0] % 100) / 100.0)
        push()
    g.replay()


for _ in range(iters):           # warm-up of the replay itself
    replay()
torch.cuda.synchronize()
blocks = []
for _ in range(5):
    t0 = time.perf_counter()
    for _ in range(iters):
        replay()
    torch.cuda.synchronize()
    blocks.append((time.perf_counter() - t0) / iters)
blocks.sort()
graph = blocks[2]
print("%s B=%d%s: eager %.2f ms = %.0f samples/s; graph replay %.3f ms (median of 5 blocks of %d; min %.3f, max %.3f) = %.0f samples/s; "
      "loss %.4f -> %.4f%s" % (name, B, " clip+schedule" if clip else "", eager * 1e3, B / eager, graph * 1e3, iters, blocks[0] * 1e3,
                               blocks[4] * 1e3, B / graph, l0, float(loss),
                               "; grad norm %.3f" % float(opt.grad_norm) if clip else ""))
