"""The reference's EAGER training loop (zero_grad, log_prob, loss, backward, step) with contextflow_amd.optim.FusedAdamW, and
every evaluation entry point after it.  FusedAdamW's kernels write parameters and moments through raw pointers; everything the
package derives from parameter values (layers/_derived.py, FlowSequential._prep, the auto-captured evaluation graphs) is keyed on
torch's version counters, so `step()` must advance the counters of what it wrote or update 2 runs on the tables of update 1.

Two references, neither of them the code under test with its history:
  * the fp64 CPU oracle (oracle.flow_oracle) at the model's CURRENT parameters - `model.state_dict()` after every update - on
    the same inputs and injected noise, gradients by torch.autograd through it.  No second training trajectory is involved;
  * a shadow: a model that has never been called, holding the live model's state_dict and the same injected noise - no call
    history, hence no cache that could be stale.  Same kernels on the same operands: compared with torch.equal, after two
    shadows agreed with each other.  (The shadows are BUILT before the live model's first call and only loaded later: building a
    model registers Parameters, which makes every flow in the process drop its caches at its next call - _Problem.shadows.)
Bars are the suite's own: 1e-5 bits/dim on logp (specialist fixtures: max(1e-5, 1e-5 |bpd|max), tests/test_gpu_parity.py);
gradients max(1e-4, 3 x the error fp32 torch.autograd makes on the same graph) of max(|ref|max, 1e-3), specialist gradients 2e-4;
the input gradient of `score` as in tests/test_score.py.
Every test also asserts, on the oracle alone, that the reference MOVED between updates by far more than the bars (20 x the logp
bar per update; 90 % of the gradient tensors by 10 x their bar): that is what makes a stale table a failure.

Inputs: the fixtures' own first 4 samples, lr = 1e-4, three updates, loss = cross-entropy of logp / D with labels arange(B) % M
(-(logp / D).mean() for one mixture)."""
import contextlib
import math

import pytest
import torch

from oracle import flow_oracle as fo
from tests.helpers import load_e2e, e2e_inputs, load_specialist, bpd

BPD_TOL = 1e-5
DEV = "cuda:0"
LR = 1e-4
B = 4
gpu = pytest.mark.gpu

FLOWS = [("mnist", None), ("cifar10", None), ("smap", "rs"), ("smap", "wave")]
FLOW_IDS = ["mnist", "cifar10", "smap-rs", "smap-wave"]


@pytest.fixture(scope="module")
def L():
    import contextflow_amd as cfa
    from contextflow_amd.layers import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return cfa.layers


# ------------------------------------------------------------------------------------------ host side (no GPU)
def test_derived_key_follows_increment_version():
    """The mechanism the optimizer relies on: `_derived.key` of a tensor is unchanged while nobody touches it and differs after
    torch.autograd.graph.increment_version - for a Parameter, and for a view through its flat base (the moments)."""
    from contextflow_amd.layers import _derived
    t = torch.zeros(5)
    p = torch.nn.Parameter(torch.ones(3))
    flat = torch.zeros(8)
    view = flat[2:6].view(2, 2)
    k0 = _derived.key((t, p, view), 3, "x")
    assert _derived.key((t, p, view), 3, "x") == k0
    torch.autograd.graph.increment_version(t)
    k1 = _derived.key((t, p, view), 3, "x")
    assert k1 != k0 and k1[1:] == k0[1:] and k1[0][1] == k0[0][1]          # only t's counter moved; same storage
    with torch.no_grad():
        torch.autograd.graph.increment_version(p)
    k2 = _derived.key((t, p, view), 3, "x")
    assert k2[1] != k1[1] and k2[0] == k1[0] and k2[2] == k1[2]
    v_flat = flat._version
    torch.autograd.graph.increment_version(view)
    assert _derived.key((t, p, view), 3, "x")[2] != k2[2] and flat._version > v_flat
    assert torch.equal(t, torch.zeros(5)) and torch.equal(p.detach(), torch.ones(3)) and torch.equal(flat, torch.zeros(8))


# ------------------------------------------------------------------------------------------ the problems and the oracle
class _Problem:
    """One fixture: oracle program, parameters, the inputs on the host; `build(sd)` makes a model with the noise injected."""

    def __init__(self, name, fxname=None):
        self.name, self.fxname = name, fxname
        if fxname is None:
            self.ops, _, self.M, self.params, fx = load_e2e(name)
            x, u, eps = e2e_inputs(name, fx)
            self.ctx = self.context = self.cnoise = None
        else:
            _, self.ctx, self.ops, self.M, self.params, inp = load_specialist(fxname)
            x, u, eps = inp["x"], inp["u"], inp["eps"]
            self.context, self.cnoise = inp["context"][:B], [c[:B] for c in inp["cnoise"]]
        assert x.shape[0] >= B
        self.x, self.u, self.eps = x[:B], (None if u is None else u[:B]), [e[:B] for e in eps]
        self.D = self.x[0].numel()
        self.labels = torch.arange(B) % self.M

    def loss(self, logp):
        lab = self.labels.to(logp.device)
        return torch.nn.functional.cross_entropy(logp / self.D, lab) if self.M > 1 else -(logp / self.D).mean()

    def build(self, sd):
        import contextflow_amd as cfa
        from tests.gpu_util import build_model
        if self.fxname is None:
            model = build_model(self.name, sd)
        else:
            ctx = self.ctx
            cfg, ds, MM = cfa.preset_config(self.name)
            cfg.update(generalist=False, enc_emb=ctx["enc_emb"], enc_type=ctx.get("enc_type", "uniform"), contextflow=ctx["contextflow"])
            model = cfa.create_model(cfg, ds, MM, contexts=ctx["contexts"])
            model.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
            model = model.to(DEV)
        self.inject(model)
        return model

    def shadows(self, n):
        """n models for ONE use each, built before the live model's first call: registering a Parameter anywhere in the process
        makes every FlowSequential drop its caches at its next call (flowsequential._PARAM_GENERATION), so a shadow built between
        two updates would hide the very staleness these tests look for.  `load` puts the live parameters in just before the use;
        `generation()` is compared at the end of every test."""
        return [self.build(self.params) for _ in range(n)]

    def load(self, model, sd):
        model.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
        self.inject(model)
        return model

    @staticmethod
    def generation():
        from contextflow_amd.layers import flowsequential as fs
        return fs._PARAM_GENERATION[0]

    def inject(self, model):
        import contextflow_amd as cfa
        from tests.gpu_util import set_noise
        set_noise(model, self.u, self.eps)
        if self.fxname is not None:
            noisy = cfa.layers.UniformCatDequantization if self.ctx.get("enc_type", "uniform") == "uniform" else cfa.layers.ConditionalGaussianDistribution
            encs = [m for m in model.modules() if isinstance(m, noisy)]
            assert len(encs) == len(self.cnoise)
            for e, c in zip(encs, self.cnoise):
                e.fixed_noise = c.to(DEV)

    def call_args(self):
        xd = self.x.to(DEV)
        return (xd,) if self.fxname is None else (xd, self.context.to(DEV))

    def oracle(self, sd, dtype=torch.float64, param_grads=False, x_grad=False):
        """logp of the oracle at the parameters `sd` (host tensors) in `dtype`; param_grads: also {name: d loss / d parameter};
        x_grad: also d sum_b logsumexp_m logp / d x (the marginal score)."""
        p = {k: (v.to(dtype).clone().requires_grad_(param_grads) if v.is_floating_point() else v) for k, v in sd.items()}
        x = self.x.to(dtype).clone().requires_grad_(x_grad)
        kw = {}
        if self.fxname is not None:
            kw = dict(ctx=self.ctx, context=self.context, cnoise=[c.to(dtype) for c in self.cnoise])
        with torch.set_grad_enabled(param_grads or x_grad):
            _, lp = fo.flow_forward(self.ops, p, x, None if self.u is None else self.u.to(dtype), [e.to(dtype) for e in self.eps], **kw)
            if param_grads:
                self.loss(lp).backward()
            elif x_grad:
                torch.logsumexp(lp, dim=1).sum().backward()
        out = [lp.detach()]
        if param_grads:
            out.append({k: v.grad for k, v in p.items() if v.is_floating_point() and v.grad is not None})
        if x_grad:
            out.append(x.grad)
        return out[0] if len(out) == 1 else tuple(out)


_PROBLEMS = {}


def _problem(name, fxname=None):
    key = (name, fxname)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = _Problem(name, fxname)
    return _PROBLEMS[key]


def _sd(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


@contextlib.contextmanager
def _step_form(form):
    """smap: 'rs' is the row-split transformer step every batch up to 3584 takes; 'wave' the one-wave-per-8-samples kernel,
    reached at a batch of 4 by moving the threshold to 0 (as test_smap_taped_backward_equals_the_recompute_form does)."""
    from contextflow_amd.layers.coupling import TransCoupling
    keep = TransCoupling.STEP_RS_MAX_BATCH
    try:
        if form == "wave":
            TransCoupling.STEP_RS_MAX_BATCH = 0
        yield
    finally:
        TransCoupling.STEP_RS_MAX_BATCH = keep


def _train_pass(prob, model):
    """zero_grad, log_prob, loss, backward on a model in train mode: (logp, {name: grad})."""
    for p in model.parameters():
        p.grad = None
    logp = model.log_prob(*prob.call_args())
    assert logp.requires_grad
    prob.loss(logp).backward()
    return logp.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}


def _assert_same(what, got, ref):
    """torch.equal over tensors / lists / dicts of tensors"""
    if isinstance(ref, dict):
        assert got.keys() == ref.keys(), (what, sorted(set(got) ^ set(ref))[:5])
        for k in ref:
            _assert_same("%s[%s]" % (what, k), got[k], ref[k])
    elif isinstance(ref, (list, tuple)):
        assert len(got) == len(ref), what
        for i, (a, b) in enumerate(zip(got, ref)):
            _assert_same("%s[%d]" % (what, i), a, b)
    else:
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        assert torch.equal(got, ref), "%s: max |difference| %.3e" % (what, (got.double() - ref.double()).abs().max().item())


def _logp_bar(prob, lp64):
    if prob.fxname is None:
        return BPD_TOL
    return max(BPD_TOL, 1e-5 * bpd(lp64.float(), prob.name).abs().max().item())       # un-normalised without contextflow


def _check_logp(what, prob, logp, lp64):
    bar = _logp_bar(prob, lp64)
    err = (bpd(logp.detach().cpu(), prob.name) - bpd(lp64.float(), prob.name)).abs().max().item()
    print("%s: |d bits/dim| vs the oracle at the current parameters %.3e = %.3f of the bar %.1e" % (what, err, err / bar, bar))
    assert err < bar, "%s: %.3e bits/dim from the oracle at the current parameters (bar %.1e)" % (what, err, bar)


def _check_moved(what, prob, lps):
    """Oracle alone: consecutive evaluations differ by more than 20 x the logp bar."""
    for i in range(1, len(lps)):
        bar = max(_logp_bar(prob, lps[i - 1]), _logp_bar(prob, lps[i]))
        moved = (bpd(lps[i], prob.name) - bpd(lps[i - 1], prob.name)).abs().max().item()
        print("%s: the oracle moved %.3e bits/dim at update %d = %.0f x the bar" % (what, moved, i, moved / bar))
        assert moved > 20.0 * bar, "%s: update %d moved the oracle by %.3e bits/dim only (bar %.1e)" % (what, i, moved, bar)


def _check_grads(what, model, grads, ref, ref32=None, fixed_bar=None, first=None, min_checked=30):
    """Every parameter's gradient against the oracle's fp64 one, relative to max(|ref|max, 1e-3); the bar of each tensor is
    `fixed_bar` or max(1e-4, 3 x its fp32 floor).  first: the oracle's gradients at the first update - at least 90 % of the tensors
    must have moved by more than 10 x their bar since."""
    checked = moved = 0
    worst = (0.0, None)
    for k, p in model.named_parameters():
        r = ref.get(k)
        if not p.requires_grad:
            assert k not in grads, k
            continue
        if r is None or float(r.abs().max()) == 0.0:            # takes no part in this configuration
            assert k not in grads or float(grads[k].abs().max()) == 0.0, k
            continue
        assert k in grads, k
        scale = max(r.abs().max().item(), 1e-3)
        err = (grads[k].detach().cpu().double() - r).abs().max().item() / scale
        bar = fixed_bar if fixed_bar is not None else max(1e-4, 3.0 * (ref32[k].double() - r).abs().max().item() / scale)
        if err / bar > worst[0]:
            worst = (err / bar, k)
        assert err < bar, "%s %s: relative gradient error %.3e (scale %.3e, bar %.1e)" % (what, k, err, scale, bar)
        checked += 1
        if first is not None and (r - first[k]).abs().max().item() / scale > 10.0 * bar:
            moved += 1
    print("%s: %d gradient tensors, worst %.3f of its bar (%s); %d moved by > 10 x the bar since the first update" % (
        what, checked, worst[0], worst[1], moved))
    assert checked >= min_checked, checked
    if first is not None:
        assert moved >= 0.9 * checked, "%s: only %d of %d oracle gradients moved" % (what, moved, checked)


# ------------------------------------------------------------------------------------------ a. training
@gpu
@pytest.mark.parametrize("form", ["host_rate", "device_rate_clipped"])
@pytest.mark.parametrize("flow", FLOWS, ids=FLOW_IDS)
def test_training_forward_and_backward_follow_eager_updates(L, flow, form):
    """Three iterations of the reference's loop in train mode.  Every iteration: the training logp against the oracle at the
    parameters it ran on, logp and every p.grad torch.equal to a shadow's; the last iteration: every gradient against fp64
    autograd through the oracle.  form: FusedAdamW(lr) = cf_adamw_step_batch; FusedAdamW(lr, max_grad_norm=X) =
    cf_adamw_step_batch_dev in eager mode, X = half the oracle's gradient norm at the first update, so that update clips."""
    import contextflow_amd as cfa
    name, step_form = flow
    prob = _problem(name)
    what = "%s %s" % (FLOW_IDS[FLOWS.index(flow)], form)
    with _step_form(step_form):
        model = prob.build(prob.params).train()
        shadows, gen = prob.shadows(4), prob.generation()
        lp0, g0 = prob.oracle(prob.params, param_grads=True)
        names = {k for k, _ in model.named_parameters()}
        X = 0.5 * math.sqrt(sum(float((g ** 2).sum()) for k, g in g0.items() if k in names))
        opt = cfa.optim.FusedAdamW(model.parameters(), lr=LR, max_grad_norm=X if form == "device_rate_clipped" else None)
        lps, norms = [], []
        for it in range(3):
            sd = _sd(model)
            logp, grads = _train_pass(prob, model)
            lp64, g64 = (lp0, g0) if it == 0 else prob.oracle(sd, param_grads=True)
            lps.append(lp64)
            _check_logp("%s iteration %d" % (what, it + 1), prob, logp, lp64)
            s_logp, s_grads = _train_pass(prob, prob.load(shadows.pop(), sd).train())
            if it == 0:                  # determinism of the reference side, once per case
                t_logp, t_grads = _train_pass(prob, prob.load(shadows.pop(), sd).train())
                _assert_same("two shadows, logp", t_logp, s_logp)
                _assert_same("two shadows, grad", t_grads, s_grads)
            _assert_same("%s iteration %d: logp vs a fresh model at the same parameters" % (what, it + 1), logp, s_logp)
            _assert_same("%s iteration %d: grad vs a fresh model at the same parameters" % (what, it + 1), grads, s_grads)
            if it == 2:
                _, g32 = prob.oracle(sd, dtype=torch.float32, param_grads=True)
                _check_grads(what, model, grads, g64, ref32=g32, first=g0)
            opt.step()
            if opt.grad_norm is not None:
                norms.append(float(opt.grad_norm))
        _check_moved(what, prob, lps)
        assert prob.generation() == gen and not shadows
        if form == "device_rate_clipped":
            print("%s: X %.4g, gradient norms %s" % (what, X, norms))
            assert len(norms) == 3 and any(n > X for n in norms), (X, norms)
        else:
            assert opt.grad_norm is None


# ------------------------------------------------------------------------------------------ b. evaluation after training
def _evaluate(prob, model, skipped, latents=None):
    """Every no_grad entry point of a generalist flow on the injected noise: log_prob, encode, decode of its latents, decode of
    the GIVEN latents (default: its own), score, sample(4) under a fixed seed.  An entry point the flow does not implement is
    recorded in `skipped` with its reason.  (decode(encode(x)) returns x through stale tables too, as long as both directions are
    equally stale: the given latents are what shows a stale inverse.)"""
    xd = prob.x.to(DEV)
    out = {}

    def entry(key, fn):
        try:
            out[key] = fn()
        except NotImplementedError as e:
            skipped[key] = "%s: %s" % (type(e).__name__, e)

    def sample():
        torch.manual_seed(1234)
        return model.sample(B)
    with torch.no_grad():
        out["logp"] = model.log_prob(xd)
        entry("encode", lambda: model.encode(xd))
        if "encode" in out:
            entry("decode", lambda: model.decode(out["encode"][0]))
            entry("decode_given", lambda: model.decode(out["encode"][0] if latents is None else latents))
        entry("score", lambda: model.score(xd))
        entry("sample", sample)
    return out


@gpu
@pytest.mark.parametrize("flow", FLOWS, ids=FLOW_IDS)
def test_evaluation_after_eager_updates_sees_the_current_parameters(L, flow):
    """Fill every evaluation cache BEFORE training (three log_prob calls at one shape on injected noise: FlowSequential._prep; three
    more on in-kernel noise: the auto-captured graph where the policy picks one; encode + decode: the inverse tables; score;
    sample), run two eager FusedAdamW updates, and after each: log_prob against the oracle at the current parameters; log_prob,
    the latents, decode(encode(x)), decode of the untrained model's latents, score and sample(4) under a fixed seed torch.equal to a
    shadow's; score's gradient against
    the oracle's d logsumexp_m logp / dx, bar max(1e-4, 3 x the fp32 floor) of |ref|max as in tests/test_score.py; log_prob on
    in-kernel noise under one seed torch.equal to the shadow's, and no captured graph older than the parameters left."""
    import contextflow_amd as cfa
    from tests.gpu_util import set_noise
    name, step_form = flow
    prob = _problem(name)
    what = FLOW_IDS[FLOWS.index(flow)]
    xd = prob.x.to(DEV)
    with _step_form(step_form):
        model = prob.build(prob.params).eval()
        shadows, gen = prob.shadows(3), prob.generation()
        skipped = {}
        with torch.no_grad():
            for _ in range(2):
                model.log_prob(xd)
        before = _evaluate(prob, model, skipped)
        set_noise(model, None, [])
        with torch.no_grad():
            for _ in range(3):
                model.log_prob(xd)
        print("%s: auto-captured graphs before training: %d" % (what, sum(st[2] is not None for st in model._graphs.values())))
        prob.inject(model)
        for key, why in skipped.items():
            print("%s: %s not checked - %s" % (what, key, why))
        assert not skipped, skipped              # (every flow here implements every entry point, smap included)
        opt = cfa.optim.FusedAdamW(model.parameters(), lr=LR)
        lps = [prob.oracle(prob.params)]
        stale = []                   # every entry point is looked at before the test fails: the message names all that are stale

        def soft(check, *a):
            try:
                check(*a)
            except AssertionError as e:
                stale.append(str(e).splitlines()[0])
        for upd in range(2):
            model.train()
            _train_pass(prob, model)
            opt.step()
            model.eval()
            sd = _sd(model)
            tag = "%s after update %d" % (what, upd + 1)
            lp64, gx64 = prob.oracle(sd, x_grad=True)
            lps.append(lp64)
            given = before["encode"][0]                  # the latents of the untrained model: the same input to both sides
            got = _evaluate(prob, model, {}, given)
            shadow = prob.load(shadows.pop(), sd).eval()
            ref = _evaluate(prob, shadow, {}, given)
            if upd == 0:
                _assert_same("two shadows", _evaluate(prob, prob.load(shadows.pop(), sd).eval(), {}, given), ref)
            assert got.keys() == before.keys() == ref.keys()
            soft(_check_logp, tag + " log_prob", prob, got["logp"], lp64)
            for key in got:
                soft(_assert_same, "%s: %s vs a fresh model at the same parameters" % (tag, key), got[key], ref[key])
            if "score" in got:
                _, gx32 = prob.oracle(sd, dtype=torch.float32, x_grad=True)
                scale = gx64.abs().max().item()
                floor = (gx32.double() - gx64).abs().max().item() / scale
                err = (got["score"][0].cpu().double() - gx64).abs().max().item() / scale
                bar = max(1e-4, 3.0 * floor)
                print("%s score: relative error %.3e = %.3f of the bar %.1e (fp32 floor %.1e)" % (tag, err, err / bar, bar, floor))
                if not err < bar:
                    stale.append("%s score: relative input-gradient error %.3e (bar %.1e)" % (tag, err, bar))
                soft(_check_logp, tag + " score's logp", prob, got["score"][1], lp64)
            # in-kernel noise: the route through the auto-captured graph
            set_noise(model, None, [])
            set_noise(shadow, None, [])
            with torch.no_grad():
                torch.manual_seed(77)
                a = model.log_prob(xd)
                torch.manual_seed(77)
                b = shadow.log_prob(xd)
            soft(_assert_same, tag + ": log_prob on in-kernel noise vs a fresh model at the same parameters", a, b)
            ver = model._versions()
            if not all(st[2] is None or st[1] == ver for st in model._graphs.values()):
                stale.append(tag + ": a captured graph older than the parameters is kept")
            prob.inject(model)
        _check_moved(what, prob, lps)
        assert prob.generation() == gen and not shadows
        assert not stale, "\n".join(stale)
        assert not torch.equal(got["logp"], before["logp"])


# ------------------------------------------------------------------------------------------ c. specialist flows
@gpu
@pytest.mark.parametrize("fxname", ["cifar10_eye", "cifar10_onehot_cf", "smap_eye", "mnist_embed_probsample_cf"])
def test_specialist_flows_follow_eager_updates(L, fxname):
    """Context-conditioned flows under three eager FusedAdamW updates, after one eval-mode no_grad forward (the grouped front end,
    specialist.forward_eval) and one train-mode forward (the taped path) have filled their tables.  cifar10_eye: nothing frozen
    (mixture tables, ctx_ws / ctx_wsb, spec_ws, spec_cnb all derive from trained tensors); cifar10_onehot_cf: the generalist
    frozen (lad / spec_lad stay valid while spec_cnb moves); smap_eye; mnist_embed_probsample_cf: the embedding tables train.
    After every update the train-mode and the eval-mode logp against the oracle at the current parameters and against a
    shadow; after the last one every trainable gradient against the oracle's (2e-4); frozen parameters keep their bits and
    get no gradient.
    Movement of the fp64 oracle at lr 1e-4, every fixture at the common rate (max over the 4 samples of |d bits/dim| per update and
    its multiple of the logp bar; gradient tensors moved by more than 10 x 2e-4 between the first and the last update).  On the
    host under fp64 torch AdamW, before any GPU run, and the same to the printed digits on the MI355X trajectory:
    cifar10_eye 0.16 / 0.22 / 0.38 = 561 / 750 / 1298 x (bar 2.9e-4), 207 of 207; cifar10_onehot_cf 2.5e-3 / 6.4e-3 / 3.0e-3 =
    30 / 79 / 37 x (bar 8.1e-5), 126 of 126; smap_eye 4.1e4 / 7.5e3 / 2.0e3 = 78 000 / 65 000 / 50 000 x (un-normalised: |bpd|
    5e4 falling to 2e3, the bar 0.52 / 0.12 / 0.04 with it), 628 of 628; mnist_embed_probsample_cf 0.032 / 0.036 / 0.040 =
    25 / 28 / 30 x (bar 1.3e-3), 268 of 269."""
    import contextflow_amd as cfa
    from tests.helpers import SPECIALIST
    prob = _problem(SPECIALIST[fxname][0], fxname)
    args = prob.call_args()

    def both(model, backward=False):
        """eval-mode no_grad logp, then train-mode logp (and its gradients)"""
        model.eval()
        with torch.no_grad():
            ev = model.log_prob(*args)
        model.train()
        if backward:
            return (ev,) + _train_pass(prob, model)
        for p in model.parameters():
            p.grad = None
        tr = model.log_prob(*args)
        assert tr.requires_grad
        return ev, tr.detach()

    model = prob.build(prob.params)
    shadows, gen = prob.shadows(4), prob.generation()
    both(model)
    initial = {k: p.detach().clone() for k, p in model.named_parameters()}
    frozen = [k for k, p in model.named_parameters() if not p.requires_grad]
    assert bool(frozen) == bool(prob.ctx["contextflow"])
    lp0, g0 = prob.oracle(prob.params, param_grads=True)
    lps = [lp0]
    opt = cfa.optim.FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=LR)
    for upd in range(3):
        _train_pass(prob, model)
        opt.step()
        sd = _sd(model)
        tag = "%s after update %d" % (fxname, upd + 1)
        last = upd == 2
        lp64 = prob.oracle(sd, param_grads=last)
        if last:
            lp64, g64 = lp64
        lps.append(lp64)
        got = both(model, backward=last)
        ref = both(prob.load(shadows.pop(), sd), backward=last)
        if upd == 0:
            _assert_same("two shadows", both(prob.load(shadows.pop(), sd)), ref)
        _check_logp(tag + " eval-mode logp", prob, got[0], lp64)
        _check_logp(tag + " train-mode logp", prob, got[1], lp64)
        _assert_same(tag + ": eval-mode logp vs a fresh model at the same parameters", got[0], ref[0])
        _assert_same(tag + ": train-mode logp vs a fresh model at the same parameters", got[1], ref[1])
        if last:
            _assert_same(tag + ": grad vs a fresh model at the same parameters", got[2], ref[2])
            _check_grads(fxname, model, got[2], g64, fixed_bar=2e-4, first=g0, min_checked=20)
    _check_moved(fxname, prob, lps)
    assert prob.generation() == gen and not shadows
    for k, p in model.named_parameters():
        if k in frozen:
            assert p.grad is None and torch.equal(p.detach(), initial[k]), k
    changed = sum(not torch.equal(p.detach(), initial[k]) for k, p in model.named_parameters() if k not in frozen)
    assert changed >= 20


# ------------------------------------------------------------------------------------------ d. the version counters
def _synthetic(max_grad_norm):
    import contextflow_amd as cfa
    g = torch.Generator().manual_seed(4)
    with_grad = [torch.nn.Parameter(torch.randn(n, generator=g).to(DEV)) for n in (1, 7, 1024, 4099)]
    idle = torch.nn.Parameter(torch.randn(33, generator=g).to(DEV))                        # grad is None
    frozen = torch.nn.Parameter(torch.randn(17, generator=g).to(DEV), requires_grad=False)
    for p in with_grad:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    opt = cfa.optim.FusedAdamW(with_grad + [idle, frozen], lr=1e-2, max_grad_norm=max_grad_norm)
    return opt, with_grad, idle, frozen


@gpu
@pytest.mark.parametrize("form", ["host_rate", "device_rate"])
def test_step_moves_the_version_counters_of_what_it_wrote(L, form):
    """After step(): p._version and the counters of exp_avg / exp_avg_sq are larger for every parameter that had a gradient, in
    both kernel forms, at every step; a parameter with grad None or requires_grad=False keeps its counter and its bits."""
    opt, with_grad, idle, frozen = _synthetic(1.0 if form == "device_rate" else None)
    keep = [idle.detach().clone(), frozen.detach().clone()]
    for _ in range(2):
        before = [(p._version, opt.state[p]["exp_avg"]._version, opt.state[p]["exp_avg_sq"]._version, p.detach().clone()) for p in with_grad]
        vi, vf = idle._version, frozen._version
        opt.step()
        for p, (vp, vm, vv, old) in zip(with_grad, before):
            assert p._version > vp and opt.state[p]["exp_avg"]._version > vm and opt.state[p]["exp_avg_sq"]._version > vv
            assert not torch.equal(p.detach(), old)
        assert idle._version == vi and frozen._version == vf
    assert torch.equal(idle.detach(), keep[0]) and torch.equal(frozen.detach(), keep[1]) and frozen not in opt.state


@gpu
def test_captured_step_moves_the_version_counters_at_capture_time_only(L):
    """capture_train_step on mnist: the eager warm-up update and the captured one run step() in Python, so every counter moves;
    a replay runs no Python and moves none (GraphedTrainStep drops the caches itself), yet it updates the parameters, and an
    evaluation after it equals a fresh model's."""
    import contextflow_amd as cfa
    prob = _problem("mnist")
    model = prob.build(prob.params).train()
    shadow, gen = prob.shadows(1)[0], prob.generation()
    xd, y = prob.x.to(DEV), prob.labels.to(DEV)
    inv = 1.0 / prob.D
    opt = cfa.optim.FusedAdamW(model.parameters(), lr=LR)
    v0 = [p._version for p in model.parameters()]
    step = model.capture_train_step(xd, lambda lp, yy: torch.nn.functional.cross_entropy(lp * inv, yy), opt, data_parallel=False)
    step(xd, y)
    v1 = [p._version for p in model.parameters()]
    assert all(b >= a + 2 for a, b in zip(v0, v1))      # the eager warm-up update (host-rate kernel) and the captured one (device-rate)
    m1 = [opt.state[p]["exp_avg"]._version for p in model.parameters()]
    old = [p.detach().clone() for p in model.parameters()]
    step(xd, y)
    torch.cuda.synchronize()
    assert [p._version for p in model.parameters()] == v1 and [opt.state[p]["exp_avg"]._version for p in model.parameters()] == m1
    assert not any(torch.equal(p.detach(), o) for p, o in zip(model.parameters(), old))
    with torch.no_grad():
        a = model.log_prob(xd)
        b = prob.load(shadow, _sd(model)).train().log_prob(xd)
    _assert_same("evaluation after a replay vs a fresh model at the same parameters", a, b)
    assert prob.generation() == gen


# ------------------------------------------------------------------------------------------ parameters unfrozen after construction
@gpu
def test_a_parameter_unfrozen_after_construction_raises(L):
    """The moments are allocated at construction for the parameters that require a gradient then.  One unfrozen later has none:
    step() says so (RuntimeError naming the remedy) before it launches anything - no KeyError, no silent skip."""
    import contextflow_amd as cfa
    a = torch.nn.Parameter(torch.ones(5, device=DEV))
    late = torch.nn.Parameter(torch.ones(3, device=DEV), requires_grad=False)
    alone = torch.nn.Parameter(torch.ones(2, device=DEV), requires_grad=False)
    for params, target in (([a, late], late), ([alone], alone)):           # beside a trainable one / a group without any
        opt = cfa.optim.FusedAdamW(params, lr=1e-2)
        target.requires_grad_(True)
        for p in params:
            p.grad = torch.ones_like(p)
        with pytest.raises(RuntimeError, match="new FusedAdamW after unfreezing"):
            opt.step()
        torch.cuda.synchronize()
        assert all(torch.equal(p.detach(), torch.ones_like(p)) for p in params)
        target.requires_grad_(False)
        target.grad = None
    opt = cfa.optim.FusedAdamW([a, late], lr=1e-2)                         # frozen again: the step runs
    opt.step()
    assert not torch.equal(a.detach(), torch.ones_like(a)) and torch.equal(late.detach(), torch.ones_like(late))
