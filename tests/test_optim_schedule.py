"""Learning-rate schedules and gradient-norm clipping of contextflow_amd.optim: the multi-tensor norm / scale kernels
(cf_grad_norm_batch, cf_grad_scale_batch), the AdamW update that reads the rate and the clipping coefficient on the device
(cf_adamw_step_batch_dev), FusedAdamW(max_grad_norm=...), optim.clip_grad_norm_, and a captured training step that follows
the reference's warm-up ramp and StepLR drop (experiment_cl.py:98-105, 135; model.py:290).

Tolerances.  The norm is accumulated in fp64 from the first product on, so the fp32 value returned is the fp64 norm rounded
once: within one fp32 ulp (1.2e-7 relative) of the host's fp64 value.  Against torch's clip_grad_norm_ (an fp32 norm): 2e-7
relative on the norm, and 2e-7 of each tensor's max on the scaled gradients (one rounding of the coefficient, one of the
product).  Everything that compares two forms of the SAME arithmetic (fused clip vs clip + step, device rate vs host rate,
captured vs eager) is bit for bit."""
import ctypes
import statistics

import pytest
import torch

DEV = "cuda:0"
gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ host side (no GPU)
def test_norm_partials_query_counts_one_workgroup_per_1024_elements():
    from contextflow_amd import build, optim
    from contextflow_amd.layers import _hip
    build.build()
    numel = [1, 1024, 1025, 0, 4097]
    arr = (ctypes.c_int64 * len(numel))(*numel)
    assert _hip.lib().cf_grad_norm_partials(len(numel), ctypes.cast(arr, ctypes.c_void_p)) == 1 + 1 + 2 + 0 + 5 == 9
    assert optim._norm_partials(numel) == 9
    assert _hip.lib().cf_grad_norm_partials(0, None) == 0
    bad = (ctypes.c_int64 * 1)(-1)
    assert _hip.lib().cf_grad_norm_partials(1, ctypes.cast(bad, ctypes.c_void_p)) < 0


def test_bad_clipping_arguments_raise_before_any_device_call():
    from contextflow_amd import optim
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            optim.FusedAdamW([], max_grad_norm=bad)
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    for nt in (1, 1.0, float("inf"), 3):
        with pytest.raises(ValueError, match="norm_type"):
            optim.clip_grad_norm_([p], 1.0, norm_type=nt)
    with pytest.raises(ValueError, match="max_norm"):
        optim.clip_grad_norm_([p], 0.0)
    with pytest.raises(TypeError, match="lr"):
        optim.FusedAdamW([], lr=torch.tensor(1e-3))
    assert torch.equal(p.grad, torch.ones(3))


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


@pytest.fixture(scope="module")
def synth():
    """The tensor set of test_fused_adamw_equals_torch_adamw (150 tensors of 1 ... 100 003 elements, six gradient sets whose
    magnitudes span 1e-3 ... 1e1 per tensor), on the host; never modified."""
    g = torch.Generator().manual_seed(3)
    sizes = [1, 2, 3, 5, 9, 64, 255, 1024, 1025, 4097, 100003] + [int(torch.randint(1, 3000, (1,), generator=g)) for _ in range(139)]
    base = [torch.randn(n, generator=g) for n in sizes]
    grads = [[torch.randn(n, generator=g) * (10.0 ** float(torch.randint(-3, 2, (1,), generator=g))) for n in sizes] for _ in range(6)]
    norms = [float(torch.sqrt(sum((t.double() ** 2).sum() for t in gr))) for gr in grads]
    return sizes, base, grads, norms


def _params(base):
    return [torch.nn.Parameter(b.clone().to(DEV)) for b in base]


def _awkward(synth):
    """Parameters with the first gradient set + an empty tensor, a parameter without gradient and a gradient that starts one
    element (4 bytes) into its storage: the scalar path of the kernels.  Returns (parameters, host gradients of those that have
    one, fp64 norm)."""
    sizes, base, grads, _ = synth
    g = torch.Generator().manual_seed(11)
    ps = _params(base)
    host = [t.clone() for t in grads[0]]
    for p, t in zip(ps, host):
        p.grad = t.to(DEV)
    empty = torch.nn.Parameter(torch.zeros(0, device=DEV))
    empty.grad = torch.zeros(0, device=DEV)
    nograd = torch.nn.Parameter(torch.ones(17, device=DEV))
    off = torch.nn.Parameter(torch.zeros(2051, device=DEV))
    t = torch.randn(2051, generator=g) * 3.0
    buf = torch.zeros(2052, device=DEV)
    buf[1:].copy_(t)
    off.grad = buf[1:]
    assert off.grad.data_ptr() % 16 == 4 and off.grad.is_contiguous()
    host.append(t)
    ref = float(torch.sqrt(sum((h.double() ** 2).sum() for h in host)))
    return ps + [empty, nograd, off], host, ref


@gpu
def test_grad_norm_is_the_fp64_norm_rounded_once(L, synth):
    """fp64 accumulation end to end: the returned fp32 norm is within one fp32 ulp (1.2e-7 relative) of sqrt(sum g^2) in fp64 on
    the host, over 153 tensors (an empty one, one without gradient and one on the unaligned scalar path among them), and two runs
    give the same bits.  A threshold far above the norm gives a coefficient of exactly 1: gradients untouched."""
    from contextflow_amd import optim
    ps, host, ref = _awkward(synth)
    before = [p.grad.clone() for p in ps if p.grad is not None]
    a = optim.clip_grad_norm_(ps, 1e30)
    b = optim.clip_grad_norm_(ps, 1e30)
    assert a.is_cuda and a.dtype == torch.float32 and a.dim() == 0
    rel = abs(float(a) - ref) / ref
    print("norm %.9g vs fp64 %.17g: rel %.3e" % (float(a), ref, rel))
    assert rel <= 1.2e-7
    assert torch.equal(a, b)
    for x, y in zip(before, [p.grad for p in ps if p.grad is not None]):
        assert torch.equal(x, y)


@gpu
def test_grad_norm_spans_several_launches(L, synth):
    """More tensors than one launch's table (224) and a tensor list whose empty members come first: 500 gradients.  Scaled
    gradients against the fp64 product: four fp32 roundings (norm, norm + 1e-6, the quotient, the product) = 4 x 2^-24 < 2.4e-7
    of each tensor's max."""
    from contextflow_amd import optim
    g = torch.Generator().manual_seed(5)
    sizes = [0, 0] + [int(torch.randint(1, 2100, (1,), generator=g)) for _ in range(498)]
    host = [torch.randn(n, generator=g) for n in sizes]
    ps = [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in sizes]
    for p, t in zip(ps, host):
        p.grad = t.to(DEV)
    ref = float(torch.sqrt(sum((h.double() ** 2).sum() for h in host)))
    got = optim.clip_grad_norm_(ps, 0.25 * ref)
    assert abs(float(got) - ref) / ref <= 1.2e-7
    coef = 0.25 * ref / (ref + 1e-6)
    for p, t in zip(ps, host):
        if t.numel():
            assert (p.grad.cpu().double() - coef * t.double()).abs().max().item() <= 2.4e-7 * t.abs().max().item()


@gpu
@pytest.mark.parametrize("factor", [0.5, 2.0])
def test_clip_grad_norm_equals_torch(L, synth, factor):
    """optim.clip_grad_norm_ against nn.utils.clip_grad_norm_ on clones.  Threshold below the norm: norms to 2e-7 relative, scaled
    gradients to 2e-7 of each tensor's max.  Threshold above: coefficient exactly 1, gradients bit for bit unchanged."""
    from contextflow_amd import optim
    ps, host, ref = _awkward(synth)
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for p, q in zip(ps, qs):
        if p.grad is not None:
            q.grad = p.grad.clone()
    before = [None if p.grad is None else p.grad.clone() for p in ps]
    mine = optim.clip_grad_norm_(ps, factor * ref)
    theirs = torch.nn.utils.clip_grad_norm_(qs, factor * ref)
    rel = abs(float(mine) - float(theirs)) / float(theirs)
    print("norm: ours %.9g torch %.9g rel %.3e" % (float(mine), float(theirs), rel))
    assert rel <= 2e-7
    worst = 0.0
    for p, q, b in zip(ps, qs, before):
        if b is None:
            assert p.grad is None
            continue
        if factor > 1.0:
            assert torch.equal(p.grad, b)
        if b.numel():
            err = (p.grad - q.grad).abs().max().item() / b.abs().max().item()
            worst = max(worst, err)
            assert err <= 2e-7, err
    print("worst scaled-gradient error / tensor max: %.3e" % worst)


@gpu
@pytest.mark.parametrize("wd,maximize", [(1e-2, False), (0.0, False), (0.3, True)])
def test_fused_clip_equals_clip_then_step(L, synth, wd, maximize):
    """FusedAdamW(max_grad_norm=X) against optim.clip_grad_norm_(..., X) followed by FusedAdamW without clipping: parameters and
    moments bit for bit after six updates (the fused form scales in a register: one fp32 product, as g.mul_(coef)), p.grad left
    unscaled.  Against torch.optim.AdamW + nn.utils.clip_grad_norm_: the bars of test_fused_adamw_equals_torch_adamw.  X = median
    of the six unclipped norms: three steps clip, three do not."""
    import contextflow_amd as cfa
    sizes, base, grads, norms = synth
    X = statistics.median(norms)
    assert any(n > X for n in norms) and any(n < X for n in norms)
    pa, pb, pc = _params(base), _params(base), _params(base)
    kw = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, maximize=maximize)
    oa, ob, oc = torch.optim.AdamW(pa, **kw), cfa.optim.FusedAdamW(pb, max_grad_norm=X, **kw), cfa.optim.FusedAdamW(pc, **kw)
    clipped = []
    for gr, want in zip(grads, norms):
        for p, q, r, gg in zip(pa, pb, pc, gr):
            p.grad, q.grad, r.grad = gg.to(DEV), gg.to(DEV), gg.to(DEV)
        torch.nn.utils.clip_grad_norm_(pa, X)
        oa.step()
        ob.step()
        got = cfa.optim.clip_grad_norm_(pc, X)
        oc.step()
        assert torch.equal(ob.grad_norm, got) and abs(float(got) - want) / want <= 1.2e-7
        clipped.append(float(got) > X)
        assert torch.equal(pb[10].grad, gr[10].to(DEV))              # the fused form leaves p.grad as the backward wrote it
    assert any(clipped) and not all(clipped), clipped
    for p, q, r in zip(pa, pb, pc):
        sa, sb, sc = oa.state[p], ob.state[q], oc.state[r]
        assert torch.equal(q, r) and torch.equal(sb["exp_avg"], sc["exp_avg"]) and torch.equal(sb["exp_avg_sq"], sc["exp_avg_sq"])
        assert torch.isfinite(q).all()
        assert (p - q).abs().max().item() <= 2e-6 * max(1.0, p.abs().max().item())
        assert (sa["exp_avg"] - sb["exp_avg"]).abs().max().item() <= 1e-6 * max(1e-3, sa["exp_avg"].abs().max().item())
        assert (sa["exp_avg_sq"] - sb["exp_avg_sq"]).abs().max().item() <= 1e-6 * max(1e-6, sa["exp_avg_sq"].abs().max().item())
        assert float(sb["step"]) == 6.0


def _schedule(lr):
    """the reference's warm-up ramp over five batches from lr / 5 (experiment_cl.py:98-105), then one StepLR drop (model.py:290)"""
    return [lr * (i + 1) / 5 for i in range(5)] + [lr * 0.1]


@gpu
def test_device_learning_rate_equals_host_learning_rate(L, synth):
    """cf_adamw_step_batch_dev (rate read from a device scalar, 1 - lr wd and lr / bc1 formed on the device) against
    cf_adamw_step_batch (rate as a host double) from equal starts, a different rate every step: parameters and moments bit
    for bit.  A step at lr = 0 leaves the parameters bit for bit unchanged and moves the moments."""
    from contextflow_amd.layers import _hip
    sizes, base, grads, _ = synth
    n = len(sizes)
    numel = (ctypes.c_int64 * n)(*sizes)
    lr_dev = torch.zeros(1, device=DEV, dtype=torch.float64)
    sets = []
    for _ in range(2):
        sets.append(([b.clone().to(DEV) for b in base], [torch.zeros(k, device=DEV) for k in sizes], [torch.zeros(k, device=DEV) for k in sizes],
                     torch.zeros(1, device=DEV)))
    lrs = _schedule(3e-3) + [0.0]
    for it, lr in enumerate(lrs):
        gs = [t.to(DEV) for t in grads[it % len(grads)]]
        snap = [[t.clone() for t in sets[1][k]] for k in range(3)]
        for dev_form, (p, m, v, step) in enumerate(sets):
            step.add_(1.0)
            A = _hip.ptr_array
            if dev_form:
                lr_dev.fill_(lr)
                _hip.call("cf_adamw_step_batch_dev", n, A(p), A(gs), A(m), A(v), ctypes.cast(numel, ctypes.c_void_p), _hip.p(step),
                          _hip.p(lr_dev), _hip.p(None), 0.9, 0.99, 1e-8, 1e-2, 0, _hip.stream())
            else:
                _hip.call("cf_adamw_step_batch", n, A(p), A(gs), A(m), A(v), ctypes.cast(numel, ctypes.c_void_p), _hip.p(step),
                          lr, 0.9, 0.99, 1e-8, 1e-2, 0, _hip.stream())
        for k in range(3):
            for a, b in zip(sets[0][k], sets[1][k]):
                assert torch.equal(a, b), (it, k)
        if lr == 0.0:
            assert all(torch.equal(a, b) for a, b in zip(snap[0], sets[1][0]))
            assert not any(torch.equal(a, b) for a, b in zip(snap[1], sets[1][1]))
            assert not any(torch.equal(a, b) for a, b in zip(snap[2], sets[1][2]))
        else:
            assert not torch.equal(snap[0][10], sets[1][0][10])
    assert all(torch.isfinite(t).all() for t in sets[1][0])


@gpu
@pytest.mark.parametrize("name", ["mnist", "cifar10"])
def test_captured_step_follows_the_schedule_and_clips(L, name):
    """capture_train_step with FusedAdamW(max_grad_norm=X) under a loop that assigns param_group['lr'] before every step (warm-up
    ramp, then a drop): losses, gradient norms and parameters of the eager loop, bit for bit, over six updates at B = 64.
    X = median gradient norm of a preliminary unclipped pass; both branches must occur.  One more replay at lr = 0 leaves every
    parameter unchanged - it would not if the rate were baked into the graph."""
    import contextflow_amd as cfa
    cfg, ds, M = cfa.preset_config(name)
    g = torch.Generator().manual_seed(8)
    B = 64
    x = torch.randint(0, 256, (B, *ds), generator=g).float().to(DEV)
    y = torch.randint(0, M, (B,), generator=g).to(DEV)
    inv = 1.0 / x[0].numel()
    loss_fn = lambda lp, yy: torch.nn.functional.cross_entropy(lp * inv, yy)
    lrs = _schedule(1e-3)

    def run(captured, max_norm):
        torch.manual_seed(0)
        m = cfa.create_model(cfg, ds, M).to(DEV)
        for q in m.sequence_modules:
            if isinstance(q, cfa.layers.Dequantization):
                q.dist.fixed_noise = torch.rand(B, *ds, generator=torch.Generator().manual_seed(9)).to(DEV)
            if isinstance(q, cfa.layers.Augment):
                q.distribution.fixed_noise = torch.randn(B, q.aug_size, ds[1], ds[2], generator=torch.Generator().manual_seed(10)).to(DEV)
        with torch.no_grad():
            m(x)
        m.train()
        opt = cfa.optim.FusedAdamW(m.parameters(), lr=1e-3, max_grad_norm=max_norm)
        step = m.capture_train_step(x, loss_fn, opt, data_parallel=False) if captured else None
        losses, norms = [], []
        for lr in lrs:
            for group in opt.param_groups:
                group["lr"] = lr
            if captured:
                losses.append(float(step(x, y).detach()))
            else:
                opt.zero_grad(set_to_none=True)
                l = loss_fn(m.log_prob(x), y)
                l.backward()
                opt.step()
                losses.append(float(l.detach()))
            norms.append(float(opt.grad_norm))
        params = [p.detach().clone() for p in m.parameters()]
        if captured:
            for group in opt.param_groups:
                group["lr"] = 0.0
            step(x, y)
            torch.cuda.synchronize()
            for a, p in zip(params, m.parameters()):
                assert torch.equal(a, p.detach())
        return losses, norms, params

    X = statistics.median(run(False, 1e30)[1])
    eager, cap = run(False, X), run(True, X)
    print(name, "X", X, "norms", eager[1], "losses", eager[0])
    assert any(n > X for n in eager[1]) and any(n <= X for n in eager[1]), (X, eager[1])
    assert eager[0] == cap[0], (eager[0], cap[0])
    assert eager[1] == cap[1], (eager[1], cap[1])
    for a, b in zip(eager[2], cap[2]):
        assert torch.equal(a, b)
    assert all(torch.isfinite(a).all() for a in eager[2])


@gpu
def test_non_finite_gradient_poisons_the_step_as_in_torch(L, synth):
    """One inf gradient element: norm inf, coefficient 0, inf * 0 = NaN in that element - the parameters are NaN exactly where
    torch.optim.AdamW after nn.utils.clip_grad_norm_ (error_if_nonfinite=False) leaves them.  No skip-step policy."""
    import contextflow_amd as cfa
    sizes, base, grads, _ = synth
    pa, pb = _params(base), _params(base)
    oa, ob = torch.optim.AdamW(pa, lr=3e-3), cfa.optim.FusedAdamW(pb, lr=3e-3, max_grad_norm=1.0)
    for k, (p, q, gg) in enumerate(zip(pa, pb, grads[0])):
        gg = gg.clone()
        if k == 10:
            gg[777] = float("inf")
        p.grad, q.grad = gg.to(DEV), gg.to(DEV)
    torch.nn.utils.clip_grad_norm_(pa, 1.0)
    oa.step()
    ob.step()
    assert torch.isinf(ob.grad_norm)
    total = 0
    for p, q in zip(pa, pb):
        assert torch.equal(torch.isnan(p), torch.isnan(q))
        total += int(torch.isnan(q).sum())
    assert total >= 1
