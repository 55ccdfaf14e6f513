"""The backward of the fused transformer flow step (Conv1x1 -> ActNorm -> TransCoupling, SMAP geometry) against fp64
torch.autograd on EVERY branch: both forward kernels (row-split / wave) as the writer of the residual-stream tape, the backward
kernel k_vit_step_bwd_rs started from that tape or re-running the layers, depth 1, 2, 3 and 6, a batch-strided step input, and
the plan edges of the grouped weight gradient cf_linear_wgrad_group (one row range per member, a few, seventeen = the reduce
kernel's unrolled 16 plus its tail, more than 64 rows per range).  The reference (tests/vit_step_fp64_ref.py) is ONE step as a
plain torch function with `depth` as an argument.  Per case: z and ld (1e-5 of scale), the tape against the reference's residual
stream at the layer boundaries (1e-5 of scale: the first direct check of the [boundary][feature][token] layout both forward
kernels must agree on), dL/dx and all 3 + 6 + 10 depth + 2 parameter gradients.  Bar per tensor: min(1e-4, max(2e-6, 4 x
floor)), floor = the larger error of two fp32 evaluations of the reference on the CPU (as written / residual features permuted)
against its fp64 run.  Measured errors: profiles/vit_step_backward_fp64.md.

The tests without the `gpu` mark run the reference against the oracle, the floors of every case, the coverage of the plan edges
by the case list, and show that restated defects (a sample dropped from the parameter gradients, gld ignored, a LayerNorm
adjoint without its second-moment term, GELU differentiated as its tanh approximation) break the bars."""
import ctypes
import functools

import pytest
import torch

from oracle import flow_oracle as fo
from tests import vit_step_fp64_ref as R

DEV = "cuda:0"
ids = lambda cases: [c.id for c in cases]


def close(a, b, tol=1e-5):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item()
    assert err <= tol * scale, "max err %.3e (scale %.3e)" % (err, scale)
    return err / scale


@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


@pytest.fixture(scope="module")
def hostlib():
    from contextflow_amd import build
    from contextflow_amd.layers import _hip
    build.build()
    return _hip.lib()


@functools.lru_cache(maxsize=2)
def _drawn(case):
    """(inputs, fp64 run with its gradients, {name: (plain floor, permuted floor)}) of a case: computed once, read-only."""
    d = R.draw(case)
    ref, fl = R.floors(d, case.depth)
    return d, ref, fl


def _report(case, what, **kv):
    print("REPORT|%s|%s|%s" % (case.id, what, "|".join("%s=%s" % (k, ("%.3e" % v) if isinstance(v, float) else v) for k, v in kv.items())))


# ================================================================================================ CPU: reference, floors, coverage
@pytest.mark.parametrize("case", [R.Case(3), R.Case(2, depth=1), R.Case(3, depth=2), R.Case(2, depth=3), R.Case(5, depth=5)], ids=lambda c: c.id)
def test_reference_equals_autograd_through_the_oracle(case, monkeypatch):
    """step_ref = torch.autograd through fo.transcoupling_fwd o fo.actnorm_fwd o fo.conv1x1_fwd in fp64, to 1e-12: outputs, dL/dx and
    every parameter gradient (71 at depth 6).  depth < 6: the oracle with layers depth.. removed (fo.vit_dims patched here only).
    The permuted form equals the plain one to 1e-12, the residual stream included."""
    d = R.draw(case)
    depth = case.depth
    ref = R.step_ref(d, depth)
    names = R.grad_names(depth)
    assert len(names) == 1 + 3 + 6 + 10 * depth + 2 and set(d["p"]) == set(names[1:])
    if depth == 6:
        assert len(names) - 1 == 71
    else:
        dims = fo.vit_dims
        monkeypatch.setattr(fo, "vit_dims", lambda sz, patch: dict(dims(sz, patch), depth=depth))
    lv = lambda t: t.detach().double().clone().requires_grad_()
    p = {k: lv(v) for k, v in d["p"].items()}
    x = lv(d["x"])
    y, l0 = fo.conv1x1_fwd(x, p["Conv1x1.NN"])
    y, l1 = fo.actnorm_fwd(y, p["ActNorm.NN_t"], p["ActNorm.NN_logs"])
    z, l2 = fo.transcoupling_fwd(y, {"0." + k: v for k, v in p.items()}, "0.", R.SZ, R.PATCH)
    ld = l0 + l1 + l2
    ((z * d["gz"].double()).sum() + (ld * d["gld"].double()).sum()).backward()
    want = dict(z=z.detach(), ld=ld.detach(), gx=x.grad, **{k: v.grad for k, v in p.items()})
    for k, w in want.items():
        assert R.rel_err(ref[k], w) <= 1e-12, (k, R.rel_err(ref[k], w))
    assert ref["stream"].shape == (depth + 1, case.B, R.NTOK, R.DIM)
    perm = R.step_ref(d, depth, perm=True)
    for k in ("z", "ld", "stream") + names:
        assert R.rel_err(perm[k], ref[k]) <= 1e-12, (k, R.rel_err(perm[k], ref[k]))


@pytest.mark.parametrize("case", R.CASES, ids=ids(R.CASES))
def test_reference_floor(case):
    """Per case, without a GPU: the floor of every tensor (fp32 against fp64 on the CPU, the larger of the plain and the permuted
    form) is at most GRAD_CAP / FLOOR_FACTOR, so that no bar is decided by the 1e-4 cap."""
    d, ref, fl = _drawn(case)
    for k in ("z", "ld", "stream"):
        assert torch.isfinite(ref[k]).all()
    _report(case, "cpu", worst_plain=max(a for a, _ in fl.values()), worst_perm=max(b for _, b in fl.values()),
            median=float(torch.tensor([max(v) for v in fl.values()]).median()))
    for k, (a, b) in fl.items():
        _report(case, "floor:" + k, plain=a, perm=b)
        assert max(a, b) <= R.GRAD_CAP / R.FLOOR_FACTOR, (case.id, k, a, b)


def _plan(lib, B, depth):
    """[(rows, S, rows per range)] of the members of the grouped weight gradient at this batch, from cf_linear_wgrad_group_ws_bytes
    alone.  The number of ranges a member is cut into depends on its own rows and on the widths of the whole group: with every
    other member at one row (one range) the size query gives S of member i; with 2^30 rows it gives the number of ranges the
    group's width allows a member (`want`), from which the rows per range follow by the stated rule (at least 64, a multiple of
    8) - and must reproduce S."""
    shapes = R.member_shapes(B, depth)
    n = len(shapes)
    arr = lambda v: (ctypes.c_int * n)(*v)
    Ks, Ns = [s[1] for s in shapes], [s[2] for s in shapes]
    per = [N * K + N for K, N in zip(Ks, Ns)]

    def ranges(i, rows_i):
        rows = [1] * n
        rows[i] = rows_i
        floats, rem = divmod(lib.cf_linear_wgrad_group_ws_bytes(arr(rows), arr(Ks), arr(Ns), n), 4)
        s, rem2 = divmod(floats - (sum(per) - per[i]), per[i])
        assert rem == 0 and rem2 == 0
        return s
    out = []
    for i, (rows, _, _) in enumerate(shapes):
        S, want = ranges(i, rows), ranges(i, 1 << 30)
        rps = (max(64, -(-rows // want)) + 7) // 8 * 8
        assert S == -(-rows // rps), (B, depth, i, rows, S, want, rps)
        out.append((rows, S, rps))
    # the whole group at its true rows: the sizes add up
    total = lib.cf_linear_wgrad_group_ws_bytes(arr([s[0] for s in shapes]), arr(Ks), arr(Ns), n)
    assert total == 4 * sum(S * p_ for (_, S, _), p_ in zip(out, per))
    return out


def test_cases_cover_the_plan_edges(hostlib):
    """The case list reaches every edge of rowgemm_plan / k_rowgemm_reduce as the step uses them, and both sides of the
    production dispatch: asserted from the library's own size query, so the coverage stays true if the plan changes."""
    from contextflow_amd.layers.coupling import TransCoupling
    plans = {}
    for case in R.CASES:
        key = (case.B, case.depth)
        if key not in plans:
            plans[key] = _plan(hostlib, *key)
            S, rps = [m[1] for m in plans[key]], [m[2] for m in plans[key]]
            print("REPORT|plan|B=%d|depth=%d|rows=%d/%d|S=%d..%d|rps=%d..%d" % (key + (plans[key][0][0], plans[key][1][0], min(S), max(S), min(rps), max(rps))))
    Ss = {k: [m[1] for m in v] for k, v in plans.items()}
    assert any(all(s == 1 for s in S) for S in Ss.values())                            # one range per member: the reduce copies
    assert any(all(1 < s < 16 for s in S) for S in Ss.values())                        # the scalar loop alone
    assert any(any(s >= 16 and s % 16 for s in S) for S in Ss.values())                # the unrolled loop together with its tail
    assert any(any(m[2] > 64 for m in v) for v in plans.values())                      # more than the 64-row minimum per range
    # the suggested batches do what they are listed for at depth 6
    assert all(s == 1 for s in Ss[(5, 6)]) and min(Ss[(17, 6)]) == 2 and 17 in Ss[(261, 6)]
    assert all(m[2] > 64 for m in plans[(3585, 6)])
    cpl = TransCoupling(R.SZ, R.PATCH)
    assert TransCoupling.STEP_RS_MAX_BATCH == 3584 and cpl.step_variant(3584) == "rs" and cpl.step_variant(3585) == "wave"
    assert any(c.B == 3585 and c.fwd_form == "wave" for c in R.CASES)
    # every (form, tape, depth) combination the issue lists
    have = {(c.depth, c.fwd_form, c.taped) for c in R.CASES}
    assert {(6, "rs", 1), (6, "rs", 0), (6, "wave", 1), (6, "wave", 0)} <= have
    assert all({(dp, "rs", 1), (dp, "rs", 0), (dp, "wave", 1)} <= have for dp in (1, 2, 3))
    assert {c.fwd_form for c in R.CASES if c.sliced} == {"rs", "wave"}
    assert any(c.gain > 1 for c in R.CASES)


DEFECT_CASES = [R.Case(5), R.Case(37), R.Case(5, depth=1), R.Case(37, gain=4.0)]


@pytest.mark.parametrize("case", DEFECT_CASES, ids=ids(DEFECT_CASES))
def test_restated_defects_break_the_bar(case):
    """The comparison can fail: four defects restated on the CPU (in fp64, so nothing but the defect differs) against the bars
    the GPU test uses for the case.  (a) the last sample missing from every parameter gradient; (b) gld ignored; (c) the LayerNorm
    adjoint without its second-moment term (rstd a constant on the way back, in every LayerNorm); (d) GELU differentiated as its
    tanh approximation, the forward exact.  Each must exceed the bar of every tensor it reaches; the factors go to
    profiles/vit_step_backward_fp64.md."""
    d, ref, fl = _drawn(case)
    depth = case.depth
    names = R.grad_names(depth)
    factor = lambda got, k: R.rel_err(got, ref[k]) / R.bar(max(fl[k]))
    # (a) the parameter gradients are sums over samples, so the defect is the last sample's own term
    last = dict(d, x=d["x"][-1:], gz=d["gz"][-1:], gld=d["gld"][-1:])
    own = R.step_ref(last, depth)
    fa = {k: factor(ref[k] - own[k], k) for k in names[1:]}
    # (b) gld enters through d ld / d log_s (everything behind the conditioner's output, dL/dx included) and the Conv1x1 /
    # ActNorm log-dets
    ng = R.step_ref(dict(d, gld=torch.zeros_like(d["gld"])), depth)
    fb = {k: factor(ng[k], k) for k in names}
    # (c) reaches everything in front of a LayerNorm's input: all but the last LayerNorm's own weight and bias
    lnd = R.step_ref(d, depth, defect="ln")
    behind_c = [k for k in names if not k.startswith(R.Q + "transformer.norm.")]
    fc = {k: factor(lnd[k], k) for k in names}
    # (d) reaches everything in front of a GELU: not the last LayerNorm, nor the last layer's second Linear (its weight gradient
    # reads the GELU's OUTPUT)
    ged = R.step_ref(d, depth, defect="gelu")
    last_fc2 = R.Q + "transformer.layers.%d.1.net.3." % (depth - 1)
    behind_d = [k for k in behind_c if not k.startswith(last_fc2)]
    fd = {k: factor(ged[k], k) for k in names}
    for tag, f, reach in (("drop_last_sample", fa, names[1:]), ("gld_ignored", fb, names), ("ln_second_moment", fc, behind_c),
                          ("gelu_tanh_adjoint", fd, behind_d)):
        worst = min(reach, key=lambda k: f[k])
        _report(case, "defect:" + tag, reached=len(reach), min_factor=float(f[worst]), at=worst,
                median_factor=float(torch.tensor([f[k] for k in reach]).median()))
        assert all(f[k] > 1 for k in reach), (tag, {k: f[k] for k in reach if not f[k] > 1})
        # ... and the tensors it does not reach are the reference's to fp64 rounding
        assert all(f[k] < 1e-6 for k in names if k in f and k not in reach), (tag, [k for k in names if k in f and k not in reach and not f[k] < 1e-6])


# ================================================================================================ GPU
def _modules(L, case, p):
    """Conv1x1, ActNorm and a TransCoupling of case.depth layers holding the case's parameters; {reference name: parameter}."""
    conv, act, cpl = L.Conv1x1(R.SZ), L.ActNorm(R.SZ), L.TransCoupling(R.SZ, R.PATCH)
    vit = cpl.NN[0]
    vit.transformer.layers = vit.transformer.layers[:case.depth]          # before anything is packed
    own = dict(cpl.named_parameters())
    assert sorted(own) == sorted(R.vit_names(case.depth))
    with torch.no_grad():
        for k, v in own.items():
            v.copy_(p[k])
        conv.NN.copy_(p["Conv1x1.NN"]); act.NN_t.copy_(p["ActNorm.NN_t"]); act.NN_logs.copy_(p["ActNorm.NN_logs"]); act.initialized.fill_(1)
    act._init_done = True
    conv, act, cpl = conv.to(DEV), act.to(DEV), cpl.to(DEV)
    params = dict(cpl.named_parameters())
    params.update({"Conv1x1.NN": conv.NN, "ActNorm.NN_t": act.NN_t, "ActNorm.NN_logs": act.NN_logs})
    return conv, act, cpl, params


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.CASES, ids=ids(R.CASES))
def test_vit_step_backward_against_fp64(L, case, monkeypatch):
    """TransCoupling.step_tables -> step_forward with a tape (cf_vit_step_fwd, the case's form) -> autograd.vstep_backward
    (cf_vit_step_bwd from the tape or from x, cf_linear_wgrad_group, cf_step_param_grads_batch): z, ld and the tape against the fp64
    run at 1e-5 of scale, dL/dx and every parameter gradient finite and within its bar, dL/dx of the data-only call bitwise equal."""
    from contextflow_amd.layers import _hip, _tape, autograd
    lib = _hip.lib()
    d, ref, fl = _drawn(case)
    B, depth = case.B, case.depth
    dev = torch.device(DEV)
    conv, act, cpl, params = _modules(L, case, d["p"])
    assert cpl.step_supported(R.SZ)
    rs = case.fwd_form == "rs"
    tables = L.TransCoupling.step_tables([(cpl, conv.NN, act.NN_t, act.NN_logs)], dev, case.fwd_form, winv=rs, bwd=rs)[0]
    assert tables.form == case.fwd_form and (tables.wsb is not None) == rs
    if case.sliced:                      # the SplitPrior case: the first half of the channels, read in place
        x = d["big"].to(DEV)[:, :R.C]
        xv, xbs = _hip.bview(x)
        assert xv.data_ptr() == x.data_ptr() and xbs == 2 * R.C * R.HW
    else:
        x = d["x"].to(DEV)
        assert _hip.bview(x)[1] == R.C * R.HW
    T = lib.cf_vit_step_tape_tokens(B)
    assert T == 4 * ((B + 31) // 32 * 32) and lib.cf_vit_step_tape_floats(B, R.C, depth) == (depth + 1) * R.DIM * T
    xtape = torch.full((lib.cf_vit_step_tape_floats(B, R.C, depth),), float("nan"), device=DEV)
    ld = torch.full((B,), 1.5, device=DEV)
    z = cpl.step_forward(x, tables, ld, xtape=xtape)
    ez, eld = close(z, ref["z"]), close(ld, 1.5 + ref["ld"])
    # ---- the tape: [boundary][feature][token = 4 sample + n]; boundary 0 (the embedding output) is left unwritten by both forms
    tape = xtape.view(depth + 1, R.DIM, T)
    assert torch.isnan(tape[0]).all()
    got_stream = tape[1:, :, :4 * B].permute(0, 2, 1).reshape(depth, B, R.NTOK, R.DIM)
    assert torch.isfinite(got_stream).all()
    etape = close(got_stream, ref["stream"][1:])
    _report(case, "forward", z=ez, ld=eld, tape=etape)
    # ---- backward
    gz, gld = d["gz"].to(DEV), d["gld"].to(DEV)
    rec = _tape.VStep(conv, act, cpl, x, tables, xtape if case.taped else None)
    grouped, seen = autograd.wgrad_group, []
    monkeypatch.setattr(autograd, "wgrad_group", lambda members, *a: seen.extend(members) or grouped(members, *a))
    gx, grads = autograd.vstep_backward(rec, gz, gld)
    # the group test_cases_cover_the_plan_edges plans for is the one that ran
    assert [(m[0].shape[0], m[0].shape[1], m[1].shape[1]) for m in seen] == R.member_shapes(B, depth)
    assert gx.shape == d["x"].shape and len(grads) == len(params) == 3 + 6 + 10 * depth + 2
    got = {"gx": gx, **{k: grads[v] for k, v in params.items()}}
    failed = []
    for k in R.grad_names(depth):
        assert torch.isfinite(got[k]).all(), (case.id, k)
        floor = max(fl[k])
        err, b = R.rel_err(got[k], ref[k]), R.bar(floor)
        _report(case, k, err=err, plain=fl[k][0], perm=fl[k][1], floor=floor, bar=b)
        if not err <= b:
            failed.append("%s: err %.3e > bar %.3e (floor %.3e)" % (k, err, b, floor))
    assert not failed, (case.id, failed)
    # the frozen-weights call: the kernel alone
    gxd, none = autograd.vstep_backward(rec, gz, gld, params=False)
    assert none is None and torch.equal(gxd, gx)
