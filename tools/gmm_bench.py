#!/usr/bin/env python3
"""Times the four entry points of the register-tiled mixture kernel (cf_gmm_logprob, cf_gmm_logprob_levels, cf_gmm_logprob_keyed,
cf_gmm_resp) between HIP events on the three mixture levels of the cifar10 flow (M, K = 10, 8; 1536 / 768 / 768 columns as channel
slices).  usage: gmm_bench.py [B ...] (default 256 16384); CONTEXTFLOW_HIP_LIB selects the library (A/B runs: one process each)"""
import ctypes, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from contextflow_amd.layers import _hip
from contextflow_amd.layers.distributions import gaussian as G

batches = [int(v) for v in sys.argv[1:]] or [256, 16384]
dev = "cuda"
L = _hip.lib()
M, K, Us, Um = 10, 8, 2, 3
LEVELS = ((1536, 3072), (768, 1536), (768, 768))
WINDOW_MS = 300.0


def timed(run):
    for _ in range(5):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    iters, ms = 20, 0.0
    while True:                                                  # grow the window to WINDOW_MS
        torch.cuda.synchronize(); e0.record()
        for _ in range(iters):
            run()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= WINDOW_MS:
            return ms * 1000 / iters
        iters = int(iters * max(2.0, 1.2 * WINDOW_MS / max(ms, 1e-3)))


gen = torch.Generator().manual_seed(0)
for B in batches:
    levels = []
    for D, wide in LEVELS:
        mG, sG, wG = torch.randn(M, K, D, generator=gen), 1 + 0.2 * torch.randn(M, K, D, generator=gen), torch.randn(M, K, generator=gen)
        x = torch.randn(B, wide, generator=gen).to(dev)[:, wide - D:]
        levels.append((x, G.gmm_prepare(mG.to(dev), sG.to(dev), wG.to(dev))))
    out = torch.empty(B, M, device=dev)
    g = torch.randn(B, M, generator=gen).to(dev)
    key_s, key_m = torch.randint(0, Us, (B,), generator=gen).to(dev), torch.randint(0, Um, (B,), generator=gen).to(dev)
    order, tiles = G._key_buckets(key_s, key_s, key_m, Us, Um)
    T = tiles.shape[0]
    for i, (x, (a, nm, cst, _, _, D)) in enumerate(levels):
        xbs = x.stride(0)
        ws = torch.empty(max(L.cf_gmm_ws_bytes(B, M, K, D), 1), device=dev, dtype=torch.uint8)
        us = timed(lambda: _hip.call("cf_gmm_logprob", _hip.p(x), _hip.p(a), _hip.p(nm), _hip.p(cst), _hip.p(out),
                                     _hip.p(ws) if L.cf_gmm_ws_bytes(B, M, K, D) else None, B, M, K, D, xbs, 0, _hip.stream()))
        print("cf_gmm_logprob        level %d D=%4d B=%5d: %8.2f us" % (i, D, B, us), flush=True)
        r = torch.empty(B, M * K, device=dev)
        wr = torch.empty(L.cf_gmm_resp_ws_bytes(B, M, K, D), device=dev, dtype=torch.uint8)
        us = timed(lambda: _hip.call("cf_gmm_resp", _hip.p(x), _hip.p(a), _hip.p(nm), _hip.p(cst), _hip.p(g), _hip.p(r), _hip.p(wr),
                                     B, M, K, D, xbs, _hip.stream()))
        print("cf_gmm_resp           level %d D=%4d B=%5d: %8.2f us" % (i, D, B, us), flush=True)
        a_tab, nm_tab = a.unsqueeze(0).repeat(Us, 1, 1), nm.unsqueeze(0).repeat(Um, 1, 1)
        cst_tab = cst.unsqueeze(0).repeat(Us, 1)
        wk = torch.empty(L.cf_gmm_keyed_ws_bytes(T, B, M, K, D), device=dev, dtype=torch.uint8)
        ks = key_s.to(torch.int32)
        us = timed(lambda: _hip.call("cf_gmm_logprob_keyed", _hip.p(x), _hip.p(a_tab), _hip.p(nm_tab), _hip.p(cst_tab), _hip.p(ks),
                                     _hip.p(tiles), _hip.p(order), _hip.p(out), _hip.p(wk), T, B, M, K, D, xbs, 0, _hip.stream()))
        print("cf_gmm_logprob_keyed  level %d D=%4d B=%5d: %8.2f us" % (i, D, B, us), flush=True)
    ld1 = torch.randn(B, generator=gen).to(dev)
    assert G.gmm_levels_ok(levels)
    n = len(levels)
    parr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    Ds = (ctypes.c_int * n)(*[lv[1][5] for lv in levels])
    xbs = (ctypes.c_int64 * n)(*[lv[0].stride(0) for lv in levels])
    wl = torch.empty(L.cf_gmm_levels_ws_bytes(n, Ds, B, M, K), device=dev, dtype=torch.uint8)
    xs, as_, nms, csts = (parr([lv[0] for lv in levels]), parr([lv[1][0] for lv in levels]), parr([lv[1][1] for lv in levels]),
                          parr([lv[1][2] for lv in levels]))
    us = timed(lambda: _hip.check(L.cf_gmm_logprob_levels(n, xs, as_, nms, csts, Ds, xbs, None, _hip.p(ld1), _hip.p(out), _hip.p(wl),
                                                          B, M, K, _hip.stream()), "cf_gmm_logprob_levels"))
    print("cf_gmm_logprob_levels all levels     B=%5d: %8.2f us" % (B, us), flush=True)
