"""FlowSequential (reference: contextflow/layers/flowsequential.py:5-68).

`forward` = sum of the layers' log-dets + the prior's log-density, shape (B, M).

Two execution modes produce the same numbers:
  * layer-by-layer (any layer list, and always the first call, because ActNorm's data-dependent
    init needs the materialised intermediates);
  * the fused plan used afterwards: pre-processing (Dequantization..LogitTransform[..Augment]) in
    one kernel, each [Squeeze ->] Conv1x1 -> ActNorm -> Coupling group in ONE fp32-MFMA kernel that
    accumulates its log-det straight into a running per-sample buffer, SplitPrior / prior GMMs
    accumulated into a running (B, M) buffer, channel splits passed by stride (no copies).
    The per-call parameter transforms (log|det W|, ActNorm folding, MFMA-fragment packing, GMM
    1/sigma tables) are tiny one-workgroup kernels: they are enqueued on a side HIP stream at the
    start of the call and joined by events, so they overlap the main stream's kernels.
Set `fused = False` on the instance to force the layer-by-layer mode.

The backward walk behind `inverse` / `sample` / `decode` is layers/inverse.py; the HIP-graph classes and the policy by which `forward`
captures and replays on its own are layers/graphs.py."""
import functools
import math

import torch
import torch.nn as nn

from . import _derived, _hip, _tape, graphs, inverse as _inv
from ._tape import step_tape
from .actnorm import ActNorm
from .augment import Augment
from .conv1x1 import Conv1x1
from . import coupling as _cpl
from .coupling import Coupling, TransCoupling, step_sources
from .dequantize import preprocess_rng_fwd, preprocessing_group
from .distributions.gaussian import (GaussianMixtureDistribution, StandardNormal, gmm_logprob, gmm_levels_ok,
                                     gmm_logprob_levels, GMM_LEVELS_MAX_BATCH)
from .distributions.uniform import UniformDistribution
from .graphs import GraphedFlow, GraphedTrainStep
from .permute_axes import PermuteAxes
from .splitprior import SplitPrior
from .squeeze import Squeeze, squeeze_op

# training: the forward step kernel tapes y0 / h1 / h2 and the backward kernel loads them (no recompute of the two big
# contractions).  False = the tape is dropped after the forward and rebuilt per step at backward time by the same kernel
# (4.5x less tape memory per step, one more forward pass of kernel time; bitwise the same gradients).
TAPE_PLANES = True


VSTEP_TAPE = True        # transformer steps in training: keep the residual-stream tape (False: the backward kernel recomputes it)

# Parameter OBJECTS can be replaced behind a flow's back (`load_state_dict(assign=True)`, `m.weight = nn.Parameter(...)`,
# parametrizations): the new tensor starts at version 0 again, so the version-counter keys of the evaluation caches would
# match stale packed tables.  Every parameter registration in the process bumps this counter (a global torch hook: one integer
# compare per forward, where walking 580 data_ptr()s would cost more than a replayed SMAP forward); a flow that sees a new
# value drops everything it derived from parameters.  Writes through `param.data` (in-place or by assignment) move neither
# the version counter nor this one: call FlowSequential.invalidate_caches() after them.
_PARAM_GENERATION = [0]


def _on_parameter_registration(module, name, param):
    _PARAM_GENERATION[0] += 1


torch.nn.modules.module.register_module_parameter_registration_hook(_on_parameter_registration)


@functools.lru_cache(maxsize=None)
def _shape_query(name, C, H, W):
    """A host-only query of the library about a step shape, asked once per process."""
    return int(getattr(_hip.lib(), name)(C, H, W))


class ContextNoise:
    """The noise of the stochastic context encoders of one flow for one batch (FlowSequential.context_noise): `tensors`, one per
    encoder in `flow.modules()` order."""

    def __init__(self, tensors):
        self.tensors = list(tensors)

    def __len__(self):
        return len(self.tensors)

    def __iter__(self):
        return iter(self.tensors)


class FlowSequential(nn.Module):
    def __init__(self, dist, *modules):
        super().__init__()
        self.dist = dist
        self.mixtures = dist.M
        for i, module in enumerate(modules):
            self.add_module(str(i), module)
        self.sequence_modules = modules
        self.fused = True
        self.step_events = None      # bench.py: list collecting (start, end, batch, C, H*W) HIP events per step-kernel launch
        self.inv_events = None       # ... per inverse-step launch (sampling)
        self._plans = {}             # input (C,H,W) -> op list
        self._side = {}              # device index -> side stream for the parameter transforms
        # evaluation (no_grad): the packed step workspaces / GMM tables are kept between calls and rebuilt only when a
        # parameter they derive from changes (keyed on the tensors' version counters; `.to()` / `_apply` drops them)
        self._prep = {}              # (plan key, op index) -> (versions, buffers)
        # launch-bound regime: after AUTO_GRAPH_AFTER identical-shape no_grad calls with unchanged parameters the fused
        # forward is captured into a HIP graph and replayed (batches up to AUTO_GRAPH_MAX_BATCH); set False to disable
        self.auto_graph = True
        self._graphs = {}            # (shape, device) -> [stable calls, versions, GraphedFlow | None]
        self._graph_policy = {}      # (shape, device) -> replaying beat eager launches when it was measured (else: stay eager)
        self._tensors = None         # parameters + buffers, collected once (_versions)
        # data-parallel training (dist.GradBucket, layers/autograd.py): the backward writes the gradients into one flat
        # bucket that p.grad views and all-reduces it segment by segment while it is still running
        self.data_parallel = False
        self._grad_bucket = None
        self._gen = _PARAM_GENERATION[0]

    def __iter__(self):
        yield from self.sequence_modules

    def __getstate__(self):              # streams / cached plans / derived tables are per-process runtime state
        self._drop_derived()
        d = self.__dict__.copy()
        d["_plans"], d["_side"], d["step_events"], d["inv_events"] = {}, {}, None, None
        d["_prep"], d["_graphs"], d["_graph_policy"], d["_tensors"] = {}, {}, {}, None
        d["_grad_bucket"] = None
        d.pop("_derived_owners", None)
        return d

    def _drop_derived(self):
        """Forget every table kept while parameters are unchanged (layers/_derived.py), the flow's own and its modules'."""
        _derived.drop(self)
        # the modules that can own derived entries: collected once per module tree (`hasattr` on 636 modules cost 1-4 ms of host
        # time per call - a captured SMAP training step at a batch of 256 takes 2 ms and ends with invalidate_caches)
        owners = self.__dict__.get("_derived_owners")
        if owners is None:
            owners = self.__dict__["_derived_owners"] = [m for m in self.modules() if isinstance(m, (TransCoupling, GaussianMixtureDistribution, Coupling, Conv1x1))]
        for m in owners:
            _derived.drop(m)

    def invalidate_caches(self):
        """Drop everything derived from parameter VALUES (packed step workspaces, mixture tables, captured graphs).  Needed
        only after writes that bypass the version counters: `param.data.copy_(...)`, a kernel that writes a parameter through its
        raw pointer, and the replay of a captured graph that updates parameters (`GraphedTrainStep` calls this itself after every
        replay).  Eager optimizer steps - torch's, and `optim.FusedAdamW.step()`, which advances the counters of what its
        kernels wrote - `load_state_dict` and `.to()` are noticed without it."""
        self._prep.clear()
        self._graphs.clear()
        self._graph_policy.clear()                   # the replay-vs-eager verdicts are measured again
        self._tensors = None                         # a Parameter OBJECT may have been replaced (load_state_dict(assign=True), m.w = nn.Parameter(..))
        self.__dict__.pop("_fusable_ok", None)       # (an ActNorm may have been reset)
        self.__dict__.pop("_all_params", None)
        self._drop_derived()

    def _apply(self, fn, *a, **k):         # .to() / .cuda() / .float(): new storages, same version counters
        self._prep, self._graphs, self._plans, self._tensors = {}, {}, {}, None
        self._grad_bucket = None
        self._drop_derived()
        return super()._apply(fn, *a, **k)

    def _versions(self):
        ts = self._tensors
        if ts is None:                       # the module tree is walked once (580 tensors in ~300 modules for the smap flow: per call
            ts = self._tensors = tuple(self.parameters()) + tuple(self.buffers())    # that walk cost more than the replayed forward)
        return tuple(t._version for t in ts)

    # ------------------------------------------------------------------ layer-by-layer mode
    def _forward_layers(self, input, context, halves=None):
        """halves, if a list, receives the channel half every SplitPrior scores and drops (`encode`)."""
        M, B = self.mixtures, input.shape[0]
        logdet = torch.zeros((B, M), device=input.device)
        for module in self.sequence_modules:
            if halves is not None and isinstance(module, SplitPrior):
                halves.append(input[:, input.shape[1] // 2:])
            input, ldj = module(input, context)
            logdet += ldj if ldj.dim() == 2 else ldj.unsqueeze(-1)      # flowsequential.py:23
        return input, self.dist.log_prob(input, context) + logdet

    # ------------------------------------------------------------------ fused plan
    def _fusable(self):
        if not self.fused or not isinstance(self.dist, GaussianMixtureDistribution):
            return False
        # a positive answer holds until the module tree changes (`_gen`) or the caches are dropped: the walk below - ~50 layers through
        # nn.Module.__getattr__ - costs 90 us of host time, per forward call, and an eager training step is host-bound
        ok = self.__dict__.get("_fusable_ok")
        if ok is not None and ok[0] == self._gen and all(a._init_done for a in ok[1]):      # (a loaded state_dict may reset an ActNorm)
            return True
        if getattr(self.dist, "context_net", None):
            return False                     # specialist models run layer by layer (per-sample parameters)
        for m in self.sequence_modules:
            if getattr(m, "context_net", None) or getattr(getattr(m, "dist", None), "context_net", None):
                return False
            if isinstance(m, ActNorm) and not m.is_initialized():
                return False
        self.__dict__["_fusable_ok"] = (self._gen, [m for m in self.sequence_modules if isinstance(m, ActNorm)])
        return True

    def _trainable_params(self):
        """The parameters with requires_grad, in `parameters()` order; the flat parameter list is kept until the module tree changes."""
        allp = self.__dict__.get("_all_params")
        if allp is None or allp[0] != self._gen:
            allp = self.__dict__["_all_params"] = (self._gen, list(self.parameters()))
        return [p for p in allp[1] if p.requires_grad]

    def _specialist(self):
        return bool(getattr(self.dist, "context_net", None))

    def _has_context_nets(self):
        """True when the prior, a layer or a layer's prior carries a context net (a specialist flow).  The answer is kept until a
        parameter is registered somewhere (the generalist `sample` / `encode` / `decode` ask per call)."""
        hit = self.__dict__.get("_ctx_nets")
        if hit is None or hit[0] != _PARAM_GENERATION[0]:
            hit = self.__dict__["_ctx_nets"] = (_PARAM_GENERATION[0], bool(getattr(self.dist, "context_net", None)) or any(
                getattr(m, "context_net", None) or getattr(getattr(m, "dist", None), "context_net", None) for m in self.sequence_modules))
        return hit[1]

    def _needs_only_init(self):
        """True when the fused plan is blocked only by ActNorm layers that have not seen their first batch yet."""
        if not self.fused or not isinstance(self.dist, GaussianMixtureDistribution):
            return False
        return not self._has_context_nets()

    def _refresh_generation(self):
        """A Parameter object was (re)registered somewhere since the last call (see _PARAM_GENERATION): drop what was derived."""
        if self._gen != _PARAM_GENERATION[0]:
            self._gen = _PARAM_GENERATION[0]
            self.__dict__.pop("_derived_owners", None)
            self.invalidate_caches()

    @staticmethod
    def _step_supported(conv, act, cpl, shape):
        if not (isinstance(conv, Conv1x1) and isinstance(act, ActNorm) and type(cpl) is Coupling):
            return False
        C, H, W = shape
        k = cpl.NN[2]
        if tuple(k.kernel_size) != (3, 3) or tuple(k.padding) != (1, 1) or conv.D != C or act.D != C:
            return False
        return bool(_hip.lib().cf_flow_step_supported(C, H, W, 3, 3))

    def _build_plan(self, shape):
        """Walk the layer list once per input shape and group it into kernels."""
        mods, n = self.sequence_modules, len(self.sequence_modules)
        ops, i = [], 0
        shape = tuple(shape)

        def is3(sh):
            return sh is not None and len(sh) == 3
        while i < n:
            m = mods[i]
            g = preprocessing_group(mods, i) if is3(shape) else None
            # the forward DRAWS the group's noise: uniform dequantisation noise only, and an Augment joins the group only when its
            # channels are standard normals (any other one runs as a layer behind it).  Injected noise is looked at per call
            if g is not None and isinstance(g.deq.dist, UniformDistribution):
                aug = g.aug if g.aug is not None and isinstance(g.aug.distribution, StandardNormal) else None
                ops.append(("pre", g, aug))
                if aug is not None:
                    shape = (shape[0] + aug.aug_size,) + shape[1:]
                i += 5 if aug is not None else 4
                continue
            if is3(shape) and i + 2 < n and self._step_supported(m, mods[i + 1], mods[i + 2], shape):
                ops.append(("step", m, mods[i + 1], mods[i + 2], shape, False))
                i += 3
                continue
            if (is3(shape) and i + 2 < n and isinstance(m, Conv1x1) and isinstance(mods[i + 1], ActNorm)
                    and isinstance(mods[i + 2], TransCoupling) and m.D == shape[0] and mods[i + 1].D == shape[0]
                    and not m.context_net and not mods[i + 1].context_net and mods[i + 2].step_supported(shape)):
                ops.append(("vstep", m, mods[i + 1], mods[i + 2], shape))       # transformer-coupling step, one kernel
                i += 3
                continue
            if isinstance(m, Squeeze) and is3(shape):
                sq = (shape[0] * m.p[0] * m.p[1], shape[1] // m.p[0], shape[2] // m.p[1])
                if (tuple(m.p) == (2, 2) and shape[1] % 2 == 0 and shape[2] % 2 == 0 and i + 3 < n
                        and self._step_supported(mods[i + 1], mods[i + 2], mods[i + 3], sq)):
                    ops.append(("step", mods[i + 1], mods[i + 2], mods[i + 3], sq, True))   # Squeeze folded in
                    i += 4
                else:
                    ops.append(("squeeze", m))
                    i += 1
                shape = sq
                continue
            if isinstance(m, SplitPrior) and isinstance(m.dist, GaussianMixtureDistribution) and is3(shape):
                ops.append(("split", m))
                shape = (shape[0] // 2,) + shape[1:]
                i += 1
                continue
            if isinstance(m, Augment) and is3(shape) and m.split_dim == 1:
                shape = (shape[0] + m.aug_size,) + shape[1:]
            elif isinstance(m, PermuteAxes) and is3(shape):
                shape = tuple(shape[a - 1] for a in m.permutation[1:])
            elif isinstance(m, (Squeeze, SplitPrior)):
                shape = None            # unknown geometry from here on: everything else runs layer by layer
            ops.append(("layer", m))
            i += 1
        return ops

    def _side_stream(self, dev, k=0):
        s = self._side.get((dev.index, k))
        if s is None:
            s = self._side[(dev.index, k)] = torch.cuda.Stream(device=dev)
        return s

    @classmethod
    def _chain_max(cls, C, H, W):
        """largest batch at which cf_flow_step_fwd_chain covers this shape (0: never)"""
        return _shape_query("cf_flow_step_chain_max_batch", C, H, W) if cls.CHAIN_STEPS else 0

    CHAIN_STEPS = True               # False: every flow step its own launch at every batch size (A/B, tests)

    def _level_min(self, C, H, W):
        """smallest batch at which cf_flow_step_fwd_level runs this shape's level in one launch (0: never)"""
        return _shape_query("cf_flow_step_level_min_batch", C, H, W) if (C, H, W) in self.LEVEL_STEPS else 0

    # shapes whose resolution level runs as ONE launch at saturating batches, z in LDS from step to step (empty: every step its
    # own launch; A/B, tests).  A shape is listed where its level launch measured faster than its step launches by more than five
    # times their run-to-run spread (profiles/level_chain.md).  (64, 4, 4) did not: 17.84 against 17.86 - 17.94 ms per level pass;
    # neither did mnist's (8, 16, 16): 5.03 against 5.12 - 5.16 ms, a gain of twice the spread of its step launches.
    LEVEL_STEPS = frozenset({(16, 16, 16), (32, 8, 8)})

    @staticmethod
    def _prepare_steps(steps, shape, dev, train=False):
        """Packed tables of SEVERAL flow steps of one shape - steps: [(conv, act, cpl)] - in one factorisation launch and one
        packing launch (cf_flow_step_prepare_batch).  train: also Wm^-1 per step (d log|det W| / dW) and the transposed
        fragments of the backward kernel (cf_flow_step_bwd_prepare_batch).  Returns [ws] or [(ws, winv, wsb)]."""
        C, H, W = shape
        L = _hip.lib()
        f, n = _hip.f32, len(steps)
        wsz = L.cf_flow_step_ws_bytes(C, H, W)
        ws = [torch.empty(wsz, device=dev, dtype=torch.uint8) for _ in range(n)]
        cols = list(zip(*[[f(t.detach()) for t in step_sources(*s)] for s in steps]))       # one column per source tensor
        A = _hip.ptr_array
        winv = [torch.empty(C, C, device=dev, dtype=torch.float32) for _ in range(n)] if train else None
        _hip.call("cf_flow_step_prepare_batch", n, *[A(c) for c in cols], A(ws), A(winv) if train else None, C, H, W, _hip.stream())
        if not train:
            return ws
        bsz = L.cf_flow_step_bwd_ws_bytes(C, H, W)
        wsb = [torch.empty(bsz, device=dev, dtype=torch.uint8) for _ in range(n)]
        _hip.call("cf_flow_step_bwd_prepare_batch", n, A(cols[0]), A(cols[2]), A(cols[3]), A(cols[5]), A(cols[7]), A(wsb), C, H, W, _hip.stream())
        return list(zip(ws, winv, wsb))

    def _tables(self, plan, key, B, dev, main, tape, data_only=False):
        """The parameter transforms of a fused call: kept from the previous call while the parameters they derive from are
        unchanged (evaluation); otherwise rebuilt on the side stream, overlapping the main stream's kernels.  Returns
        (prepared: plan index -> (buffers, producer's event | None), prior tables, their event | None, fresh: the entries built
        by THIS call).

        `_prep` has a rule of its own (not layers/_derived.py's): a HIT is allowed while capturing, without the event wait.  A
        capturing stream must not wait on an event recorded outside the capture - and need not: torch.cuda.graph synchronises
        the device before the capture begins, so cached tables are complete by then.  GraphedFlow depends on it: it warms the
        cache up before it captures, and its graph then holds no prepare launches.  Tables built DURING a capture live in the
        graph's private pool and their events belong to the capture: they must not outlive it as cache entries (a later eager
        call would wait on a captured event and read buffers that only exist after a replay), so a user-side capture with a
        cold cache simply rebuilds the tables inside its graph.
        data_only (the input gradient with frozen weights: `score`, a frozen model under autograd): the training form of the
        step tables - with the backward kernel's fragments - is kept the same way, in slots of its own."""
        prepared, todo, vkey = {}, [], {}
        cache_ok = tape is None or data_only
        slot = lambda k, op: (key, k, vkey.get(k)) + (("train",) if tape is not None and op[0] in ("step", "vstep") else ())
        capturing = torch.cuda.is_current_stream_capturing()
        store_ok = cache_ok and not capturing
        for k, op in enumerate(plan):
            if op[0] == "step":
                srcs = step_sources(op[1], op[2], op[3])
            elif op[0] == "vstep":
                srcs = (op[1].NN, op[2].NN_t, op[2].NN_logs) + op[3].step_sources()
                vkey[k] = op[3].step_variant(B)      # small / saturating batches: two kernels, two fragment layouts
            elif op[0] == "split":
                srcs = (op[1].dist.mG, op[1].dist.sG, op[1].dist.wG)
            else:
                continue
            ver = _derived.key(srcs, dev.index)
            hit = self._prep.get(slot(k, op)) if cache_ok else None
            if hit is not None and hit[0] == ver:
                prepared[k] = (hit[1], None if capturing else hit[2])      # the producer's event stays with the entry: a later call on ANOTHER
            else:                                    # stream is ordered against the side stream that wrote the buffers
                todo.append((k, op, ver))
        pver = _derived.key((self.dist.mG, self.dist.sG, self.dist.wG), dev.index)
        hit = self._prep.get((key, "prior")) if cache_ok else None
        prior, ev_prior = (hit[1], None if capturing else hit[2]) if (hit is not None and hit[0] == pver) else (None, None)
        fresh = set()                # (their buffers get a record_stream at the end of the call: _consumed_on)
        if not todo and prior is not None:
            return prepared, prior, ev_prior, fresh
        # (one side stream: spreading the tables of the flow steps over 2 / 4 streams was measured on the captured training
        # step at a batch of 256 - smap 2.10 -> 2.16 ms, cifar10 2.49 -> 2.48 ms: tools/dev/prep_streams_ab.py - and dropped)
        side = self._side_stream(dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            # conv steps: the tables of all steps of one shape in ONE factorisation + ONE packing launch (+ one for the
            # backward kernel's fragments when training) - cf_flow_step_prepare_batch
            groups = {}
            for k, op, ver in todo:
                if op[0] == "step":
                    groups.setdefault(tuple(op[4]), []).append((k, op, ver))
            # (one event per group, recorded right behind its launches: the first level's steps start as soon as THEIR
            # tables exist - the 64-channel factorisation alone takes 50 us - instead of behind every table of the flow)
            done, done_ev = {}, {}
            for shape, items in groups.items():
                bufs = self._prepare_steps([(it[1][1], it[1][2], it[1][3]) for it in items], shape, dev, train=tape is not None)
                gev = torch.cuda.Event()
                gev.record(side)
                for (k, op, ver), buf in zip(items, bufs):
                    done[k] = buf
                    done_ev[k] = gev
            # transformer steps (TransCoupling.step_tables) at small batches: the row-split tables of all steps in one launch
            # triple (training: with Wm^-1 and the backward kernel's tables); at saturating batches: a step at a time, below
            vitem = lambda op: (op[3], op[1].NN, op[2].NN_t, op[2].NN_logs)
            vitems = [(k, op, ver) for k, op, ver in todo if op[0] == "vstep" and vkey[k] == "rs"]
            if vitems:
                train = tape is not None
                bufs = TransCoupling.step_tables([vitem(it[1]) for it in vitems], dev, "rs", winv=train, bwd=train)
                gev = torch.cuda.Event()
                gev.record(side)
                for (k, op, ver), buf in zip(vitems, bufs):
                    done[k] = buf
                    done_ev[k] = gev
            for k, op, ver in todo:
                if k in done:
                    buf, ev = done[k], done_ev[k]
                else:
                    if op[0] == "vstep":
                        buf = TransCoupling.step_tables([vitem(op)], dev, vkey[k])[0]
                    else:
                        buf = op[1].dist.prepared()
                    ev = torch.cuda.Event()
                    ev.record(side)
                prepared[k] = (buf, ev)
                fresh.add(k)
                if store_ok:
                    self._prep[slot(k, op)] = (ver, buf, ev)
            if prior is None:
                prior = self.dist.prepared()
                ev_prior = torch.cuda.Event()
                ev_prior.record(side)
                fresh.add("prior")
                if store_ok:
                    self._prep[(key, "prior")] = (pver, prior, ev_prior)
        return prepared, prior, ev_prior, fresh

    @staticmethod
    def _consumed_on(main, prepared, prior, fresh):
        """Buffers written on the side stream by this call are consumed on the main stream: keep the allocator informed."""
        def bufs(t):
            if torch.is_tensor(t):
                yield t
            elif isinstance(t, tuple):
                for u in t:
                    yield from bufs(u)

        for k in fresh:
            for buf in bufs(prior if k == "prior" else prepared[k][0]):
                buf.record_stream(main)

    def _forward_fused(self, x, context, tape=None, halves=None, data_only=False):
        """halves, if a list, receives the channel slice every SplitPrior's mixture kernel scores, in forward order (`encode`).
        tape, if a list, receives the records of layers/_tape.py (the taping kernels run); data_only: the tape is for the
        data-only walk (autograd.input_gradient) - of a conv step it keeps the aux buffer alone, neither planes nor input."""
        B, M, dev = x.shape[0], self.mixtures, x.device
        key = tuple(x.shape[1:])
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = self._build_plan(key)
        main = torch.cuda.current_stream(dev)
        prepared, prior, ev_prior, fresh = self._tables(plan, key, B, dev, main, tape, data_only)

        def chain_run(k, ws, nmax, joins):
            """Plan indices and tables of the run of at most nmax steps that starts at step k (tables ws) and goes on while
            joins(next op) holds; the main stream waits on the members' tables."""
            run = [k]
            while len(run) < nmax and run[-1] + 1 < len(plan) and joins(plan[run[-1] + 1]):
                run.append(run[-1] + 1)
            tabs = [ws]
            for j in run[1:]:
                wj, evj = prepared[j]
                if evj is not None:
                    main.wait_event(evj)
                tabs.append(wj)
            return run, tabs

        # running log-dets: per-sample scalar terms / per-mixture terms (priors).  The first writer ASSIGNS (no zero-fill
        # launches): the pre-processing kernel for ld1, the first mixture kernel for ldM
        ld1 = (torch.empty if plan and plan[0][0] == "pre" else torch.zeros)(B, device=dev, dtype=torch.float32)
        ldM = torch.empty(B, M, device=dev, dtype=torch.float32)
        ldM_set = False
        levels = [] if tape is None and B <= GMM_LEVELS_MAX_BATCH else None
        st = _hip.stream()
        chained = set()              # plan indices that ran as the tail of a chained launch
        for k, op in enumerate(plan):
            kind = op[0]
            if k in chained:
                continue
            if kind == "pre":
                _, g, aug = op
                deq, n1, n2 = g.deq, g.n1, g.n2
                xin = _hip.f32(x)
                C, H, W = xin.shape[1:]
                N = C * H * W
                ldp = ld1 if k == 0 else torch.empty_like(ld1)         # the kernel assigns its per-sample ldj
                y = preprocess_rng_fwd(xin, g, aug, ldp)         # noise drawn inside the kernel ...
                rng = y is not None
                if not rng:                                            # ... or injected / odd sizes: noise tensors from the layers
                    ca = aug.aug_size if aug is not None else 0
                    y = torch.empty(B, C + ca, H, W, device=dev, dtype=torch.float32)
                    cst = -N * math.log(n1._s) - N * math.log(n2._s)      # normalize.py:42-49, twice
                    u = _hip.f32(deq.dist.sample(B, context=xin)[0])
                    _hip.call("cf_preprocess_fwd", _hip.p(xin), _hip.p(u), _hip.p(y), _hip.p(ldp), B, N, (C + ca) * H * W,
                              n1._t, n1._s, n2._t, n2._s, cst, st)
                if ldp is not ld1:
                    ld1 += ldp
                if aug is not None and not rng:
                    eps, logq = aug.distribution.sample(B)
                    y[:, C:].copy_(eps)
                    ld1 -= logq.squeeze(-1)                            # Augment ldj = -log q(eps)
                if tape is not None:
                    tape.append(_tape.Pre(y, N, n1._s, n2._s))
                x = y
            elif kind == "step":
                _, conv, act, cpl, (C, H, W), sq = op
                ws, ev = prepared[k]
                if ev is not None:
                    main.wait_event(ev)
                if tape is not None:
                    ws, winv, wsb = ws
                    # training: the taping forward kernel writes the step tape and the backward kernel reads it.  If the
                    # planes of this step would take more than 1/64 of the device memory (huge batches), or with
                    # TAPE_PLANES = False, the tape is NOT kept (4.5x less memory per step): the backward then re-runs this
                    # very kernel from the step input.  The forward is the taping kernel in both cases, so the masks the
                    # backward uses are bit for bit those of the forward that produced the loss.
                    keep = TAPE_PLANES and 18 * B * C * H * W <= torch.cuda.get_device_properties(dev).total_memory // 64
                    planes = step_tape(B, C, H, W, dev)
                    if data_only:
                        # the y0 / h1 / h2 planes are scratch here (handed back to the allocator behind the launch: the next
                        # step of the shape gets the same blocks); the walk back reads the aux buffer alone
                        tape.append(_tape.Step(conv, act, cpl, (C, H, W), sq, wsb=wsb, aux=planes[3]))
                    else:
                        tape.append(_tape.Step(conv, act, cpl, (C, H, W), sq, x, ws, winv, planes if keep else None, wsb))
                    x, xbs = _hip.bview(x)
                    z = torch.empty(B, C, H, W, device=dev, dtype=torch.float32)
                    _hip.call("cf_flow_step_fwd_taped", _hip.p(x), _hip.p(z), _hip.p(ld1), _hip.p(ws), _hip.p(planes[0]),
                              _hip.p(planes[1]), _hip.p(planes[2]), _hip.p(planes[3]), B, C, H, W, xbs, int(sq), st)
                    del planes
                    x = z
                    continue
                x, xbs = _hip.bview(x)
                z = torch.empty(B, C, H, W, device=dev, dtype=torch.float32)
                events = self.step_events
                # this step and the following ones of its shape (a resolution level) in ONE launch: the chain kernel at small batches (never
                # under step_events), the level kernel - z in LDS from step to step - at saturating ones; the run is formed only for those
                chain = events is None and 0 < B <= self._chain_max(C, H, W)
                level = not chain and 0 < self._level_min(C, H, W) <= B
                same = lambda nxt: nxt[0] == "step" and tuple(nxt[4]) == (C, H, W) and not nxt[5]
                run, tabs = chain_run(k, ws, 4, same) if chain or level else ([k], [ws])
                if len(run) > 1 and chain:
                    _hip.call("cf_flow_step_fwd_chain", _hip.p(x), _hip.p(z), _hip.p(ld1), _hip.ptr_array(tabs), len(run), B, C, H, W, xbs,
                              int(sq), st)
                elif len(run) > 1:
                    with _hip.probe(events, main, B, C, H * W):
                        _hip.call("cf_flow_step_fwd_level", _hip.p(x), _hip.p(z), _hip.p(ld1), _hip.ptr_array(tabs), len(run), B, C, H, W, xbs,
                                  int(sq), 0, st)
                    if events is not None:   # one record per step all the same: the first carries the launch, the others are empty
                        events.extend([(events[-1][1], events[-1][1], B, C, H * W)] * (len(run) - 1))
                else:
                    with _hip.probe(events, main, B, C, H * W):
                        _hip.call("cf_flow_step_fwd", _hip.p(x), _hip.p(z), _hip.p(ld1), _hip.p(ws), B, C, H, W, xbs, int(sq), st)
                chained.update(run[1:])
                x = z
            elif kind == "vstep":
                tables, ev = prepared[k]
                if ev is not None:
                    main.wait_event(ev)
                if tape is not None:         # training: the same one-kernel forward; the backward re-runs the step from its input
                    #                          (and reuses the packed tables when they are the row-split ones)
                    # the residual stream at the layer boundaries goes to a tape (5.8 KB per sample and step) and the backward
                    # kernel does not run the six layers a second time
                    xt = None
                    if VSTEP_TAPE:
                        depth = len(op[3].NN[0].transformer.layers)
                        xt = torch.empty(_hip.lib().cf_vit_step_tape_floats(B, x.shape[1], depth), device=dev, dtype=torch.float32)
                    tape.append(_tape.VStep(op[1], op[2], op[3], x, tables, xt))
                    x = op[3].step_forward(x, tables, ld1, xtape=xt)
                    continue
                if self.CHAIN_STEPS and tables.form == "rs" and _cpl.VIT_EVENTS is None:
                    # small batch (row-split form): this step and the transformer steps that follow it in ONE launch
                    depth = len(op[3].NN[0].transformer.layers)
                    run, tabs = chain_run(k, tables, int(_hip.lib().cf_vit_step_chain_max_steps()),
                                          lambda nxt: (nxt[0] == "vstep" and nxt[3].step_variant(B) == "rs"
                                                       and len(nxt[3].NN[0].transformer.layers) == depth))
                    if len(run) > 1:
                        xv, xbs = _hip.bview(x)
                        z = torch.empty(B, xv.shape[1], xv.shape[2], xv.shape[3], device=dev, dtype=torch.float32)
                        _hip.call("cf_vit_step_fwd_chain", _hip.p(xv), _hip.p(z), _hip.p(ld1), _hip.ptr_array([tb.ws for tb in tabs]), len(run), B,
                                  xv.shape[1], depth, xbs, st)
                        chained.update(run[1:])
                        x = z
                        continue
                x = op[3].step_forward(x, tables, ld1)
            elif kind == "squeeze":
                if tape is not None:
                    tape.append(_tape.Squeeze(tuple(op[1].p)))
                x = squeeze_op(x, op[1].p, False)
            elif kind == "split":
                prep, ev = prepared[k]
                if ev is not None:
                    main.wait_event(ev)
                if tape is not None:
                    tape.append(_tape.Split(op[1].dist, x, prep))
                c = x.shape[1] // 2
                if halves is not None:
                    halves.append(x[:, c:])
                if levels is not None:       # small batch: every mixture of the flow in one launch pair at the end
                    levels.append((x[:, c:], prep))
                else:
                    gmm_logprob(x[:, c:], prep, out=ldM, accumulate=ldM_set)
                    ldM_set = True
                x = x[:, :c]
            else:                        # any other layer: its own kernels
                if tape is not None:
                    tape.append(_tape.Layer(op[1], x))
                if halves is not None and isinstance(op[1], SplitPrior):
                    halves.append(x[:, x.shape[1] // 2:])
                x, ldj = op[1](x, context)
                if ldj.dim() == 2:
                    if ldM_set:
                        ldM += ldj
                    else:
                        ldM.copy_(ldj.expand_as(ldM))
                        ldM_set = True
                else:
                    ld1 += ldj
        if ev_prior is not None:
            main.wait_event(ev_prior)
        if tape is not None:
            tape.append(_tape.Prior(self.dist, x, prior))
        if levels is not None and gmm_levels_ok(levels + [(x, prior)]):
            logp = gmm_logprob_levels(levels + [(x, prior)], ldM if ldM_set else None, ld1)
        else:
            for xl, prep in levels or ():
                gmm_logprob(xl, prep, out=ldM, accumulate=ldM_set)
                ldM_set = True
            gmm_logprob(x, prior, out=ldM, accumulate=ldM_set)
            logp = torch.empty(B, M, device=dev, dtype=torch.float32)
            _hip.call("cf_logdet_combine", _hip.p(ldM), _hip.p(ld1), _hip.p(logp), B, M, st)
        self._consumed_on(main, prepared, prior, fresh)
        return x, logp

    # ------------------------------------------------------------------ reference API
    def forward(self, input, context=None):
        _hip.require_device(input)
        self._refresh_generation()
        if torch.is_grad_enabled() and self._specialist():
            from .autograd_ctx import trainable as _trainable
            params = self._trainable_params()
            # specialist training under contextflow (autograd_ctx.py), and d logp / d x for an input that requires a gradient - also
            # from a frozen or eval() specialist (the data-only walk); other specialist models evaluate only: they fall through
            # to the no_grad path
            if (params or (input.requires_grad and context is not None)) and _trainable(self):
                if any(isinstance(m, ActNorm) and m.contextflow and not m.is_initialized() for m in self.sequence_modules):
                    with torch.no_grad():    # first call: the ActNorm data-dependent init
                        self._forward_layers(input, context)
                from .autograd_ctx import SpecialistLogProb
                return SpecialistLogProb.apply(self, input, context, *params)
        if torch.is_grad_enabled():
            params = self._trainable_params()
            if params and not self._fusable() and self._needs_only_init():
                with torch.no_grad():        # first training call: the ActNorm data-dependent init (actnorm.py:28-35)
                    self._forward_layers(input, context)
            # training: same kernels + a tape, hand-written backward (autograd.py); an input that requires a gradient gets
            # d logp / d x the same way - also from a frozen or eval() model (the data-only walk)
            if (params or input.requires_grad) and self._fusable():
                from .autograd import FlowLogProb
                return FlowLogProb.apply(self, input, *params)
        with torch.no_grad():
            if self._fusable():
                g = graphs._auto_graph(self, input)
                if g is not None:
                    z, logp = g(input)
                    return z.clone(), logp.clone()       # the graph's static outputs are overwritten by the next replay
                return self._forward_fused(input, context)
            if self.fused and self._specialist():
                from . import specialist
                if specialist.supported(self):       # grouped evaluation plan of the specialist conv flows
                    return specialist.forward_eval(self, input, context)
            return self._forward_layers(input, context)

    AUTO_GRAPH_AFTER = graphs.AUTO_GRAPH_AFTER           # graphs._auto_graph reads both through the flow:
    AUTO_GRAPH_MAX_BATCH = graphs.AUTO_GRAPH_MAX_BATCH   # settable on the class or on an instance

    def capture_train_step(self, example_input, loss_fn, optimizer, warmup=1, data_parallel=None):
        """One whole training step - forward, loss, hand-written backward, optimizer update - captured into ONE HIP graph
        (at the reference's batch of 256 a step is ~330 launches of a few microseconds each: launch-bound).  Returns
        `step(x, *loss_args) -> loss` that copies its arguments into static buffers and replays; `loss_fn(logp, *loss_args)`
        maps the (B, M) log-densities to a scalar.  The optimizer must be capturable (`torch.optim.AdamW(..., capturable=
        True)`, or `optim.FusedAdamW`).  Learning-rate schedules: only `optim.FusedAdamW` follows `param_group['lr']` after the
        capture (assign Python floats; its `max_grad_norm` is the reference's `clip_grad_norm_` inside the step);
        `torch.optim.AdamW` with a float `lr` keeps the rate it was captured with for ever.  ActNorm layers must be
        initialised (run one forward first).  The first call runs `warmup` eager steps (real updates; default 1) and
        captures; see GraphedTrainStep.
        data_parallel (default: whether a process group of more than one rank exists): every rank steps on ITS shard of the
        batch and the gradients are averaged over the ranks inside the step - written by the backward kernels into one flat
        bucket that `p.grad` views, all-reduced (RCCL) segment by segment while the backward of the lower levels still runs,
        the optimizer waits for the last one; the collectives are captured with the step (`self.data_parallel`,
        dist.GradBucket)."""
        if data_parallel is None:
            from .. import dist as cdist
            data_parallel = cdist._active()
        self.data_parallel = bool(data_parallel)
        return GraphedTrainStep(self, example_input, loss_fn, optimizer, warmup)

    def log_prob(self, input, context=None):
        return self.forward(input, context)[1]

    def score(self, x, labels=None, weights=None, context=None):
        """(grad, logp): grad = d/dx sum_m w[b, m] logp[b, m], fp32 in the shape of x, and the (B, M) log-densities.
        weights: the (B, M) tensor w, used as given.  labels: an int or B class indices - one-hot rows (checked as `sample`
        checks them: ValueError for host values outside [0, M) or a wrong length).  Neither: the score of the marginal,
        d/dx log sum_m p(x | m), i.e. w = softmax(logp, dim=1) of the returned logp.  Both: ValueError.
        Always the data-only walk (the kernels of `forward`, a tape of the steps' aux buffers, the data halves of the backward:
        layers/autograd.input_gradient), whatever the parameters' requires_grad; works under no_grad and touches no .grad
        and no requires_grad.  Generalist flows on the fused plan; specialist flows with their `context` (the (B, nctx) integer
        tensor `forward` takes) through autograd_ctx.taped_forward / input_gradient_ctx - the context encoders draw their noise as
        `forward` does, it is a constant of the gradient and its log-density enters logp alone.  NotImplementedError otherwise."""
        _hip.require_device(x)
        if labels is not None and weights is not None:
            raise ValueError("score: give labels or weights, not both")
        self._refresh_generation()
        specialist = self._has_context_nets()
        if specialist:
            from . import autograd_ctx
            if context is None:
                raise NotImplementedError("score of a context-conditioned (specialist) flow needs its context")
            if not self._specialist() or not autograd_ctx.trainable(self):
                raise NotImplementedError("score of a specialist flow: a context encoder or layout the taped forward is not built for")
            if any(isinstance(m, ActNorm) and m.contextflow and not m.is_initialized() for m in self.sequence_modules):
                raise NotImplementedError("score needs initialised ActNorms (run one forward first)")
        elif not self._fusable():
            raise NotImplementedError("score needs the fused plan: a mixture prior, initialised ActNorms (run one forward first) and fused = True")
        from .autograd import input_gradient
        B, M = x.shape[0], self.mixtures
        xd = x.detach()
        if specialist and B == 0:        # empty batch: nothing to launch
            return xd.new_zeros(x.shape, dtype=torch.float32), xd.new_zeros((0, M), dtype=torch.float32)
        if labels is not None:
            lab, m = self.dist._class_labels(labels, B)
            if lab is None:
                lab = torch.full((B,), m, device=xd.device, dtype=torch.int64)
            weights = torch.nn.functional.one_hot(lab.to(torch.int64).clamp(0, M - 1), M).to(torch.float32)
        elif weights is not None:
            if tuple(weights.shape) != (B, M):
                raise ValueError("score: weights of shape %s, (%d, %d) expected" % (tuple(weights.shape), B, M))
            weights = weights.detach().to(device=xd.device)
        with torch.no_grad():
            if specialist:
                _, logp, tape = autograd_ctx.taped_forward(self, xd, context, data_only=True)
            else:
                tape = []
                _, logp = self._forward_fused(xd, None, tape=tape, data_only=True)
            if weights is None:
                weights = torch.softmax(logp, dim=1)
            grad = (autograd_ctx.input_gradient_ctx if specialist else input_gradient)(tape, weights).reshape(x.shape)
        return grad, logp

    def capture(self, example_input):
        """Capture the fused forward for inputs of this exact shape into a HIP graph; returns a callable
        `g(x) -> (z, logp)` (static output buffers, overwritten by the next replay)."""
        return GraphedFlow(self, example_input)

    # ------------------------------------------------------------------ the stochastic context encoders, pinned
    def _stochastic_encoders(self):
        """Every module of the flow that draws noise when it encodes a context, in `modules()` order."""
        from .context import ConditionalGaussianDistribution, UniformCatDequantization
        return [m for m in self.modules() if isinstance(m, (UniformCatDequantization, ConditionalGaussianDistribution))]

    def context_noise(self, context):
        """One noise tensor per stochastic context encoder of the flow - every UniformCatDequantization ((B, width) uniforms) and
        every ConditionalGaussianDistribution ((B, D) normals), in `modules()` order, in the shapes those encoders draw, from
        torch's device generator - as a ContextNoise.  Passed as `noise=` to encode / decode / inverse / sample it makes both
        directions see the same codes: every layer of a specialist flow draws its own noise otherwise, and `decode(encode(x, c), c)`
        would not be a round trip."""
        from .context import UniformCatDequantization
        B = int(context.shape[0])
        dev = next(self.parameters()).device
        _hip.require_device(next(self.parameters()))
        out = []
        for e in self._stochastic_encoders():
            draw = torch.rand if isinstance(e, UniformCatDequantization) else torch.randn
            out.append(draw((B, e.D), device=dev, dtype=torch.float32))
        return ContextNoise(out)

    def _pinned(self, noise, context):
        """Context manager: every stochastic encoder reads its tensor of `noise` (a ContextNoise, or a sequence of tensors in
        the same order) for the duration of the block; an encoder whose `fixed_noise` is already set keeps it.  None: nothing."""
        import contextlib

        @contextlib.contextmanager
        def pin():
            encs = self._stochastic_encoders()
            tensors = list(noise.tensors if isinstance(noise, ContextNoise) else noise)
            if len(tensors) != len(encs):
                raise ValueError("noise: %d tensors for a flow with %d stochastic context encoders" % (len(tensors), len(encs)))
            B = None if context is None else int(context.shape[0])
            for e, t in zip(encs, tensors):
                if t.dim() != 2 or t.shape[1] != e.D or (B is not None and t.shape[0] != B):
                    raise ValueError("noise: a tensor of shape %s for an encoder that draws (%s, %d)" % (tuple(t.shape), B, e.D))
            mine = [(e, t) for e, t in zip(encs, tensors) if e.fixed_noise is None]
            try:
                for e, t in mine:
                    e.fixed_noise = t
                yield
            finally:
                for e, _ in mine:
                    e.fixed_noise = None
        return contextlib.nullcontext() if noise is None else pin()

    def _need_context(self, what, context):
        if context is None and self._has_context_nets():
            raise ValueError("%s: a context-conditioned (specialist) flow needs its context" % what)

    def _refuse_differentiable(self, what, context, clamp, return_logp):
        """What `inverse` / `decode` with differentiable=True (layers/autograd_inverse.py) do not take."""
        if clamp:
            raise ValueError("%s: clamp=True together with differentiable=True - the clamp is about pixels, the differentiable walk "
                             "returns the continuous point in front of the floor" % what)
        if return_logp:
            raise NotImplementedError("%s: return_logp=True together with differentiable=True" % what)
        if self._has_context_nets():
            # a specialist flow: its context is required as everywhere; the walk refuses, by name and index, a context
            # layer it has no rule for (TransCoupling, a Coupling outside the fused geometry)
            self._need_context(what, context)
        elif context is not None:
            raise NotImplementedError("%s: differentiable=True with a context for a flow without context nets" % what)

    def _run_differentiable(self, z, latents, context, noise):
        from . import autograd_inverse
        if not self._has_context_nets():
            return autograd_inverse.run(self, z, latents)
        with self._pinned(noise, context):               # the codes are formed once, here; backward reads the records
            return autograd_inverse.run(self, z, latents, context)

    def inverse(self, z, context=None, noise=None, return_logp=False, differentiable=False):
        """Run every layer's `reverse` from the last to the first (the loop of flowsequential.py:35-37); groups
        Coupling <- ActNorm <- Conv1x1 of a supported shape run as one fused kernel.  A specialist flow takes its `context`
        (ValueError without): ActNorm(c) <- Conv1x1(c) pairs, with the Squeeze((2,2)) in front of them, run as one
        cf_affine_ctx_inv launch, the couplings layer by layer; noise (`context_noise`): the codes the encoders form.
        return_logp: (x, logp) with logp (B, M) fp32 - what `forward` returns at the continuous point the walk passes through,
        the noise layers given the noise this walk implies (the dequantisation noise is the fractional part the floor drops, the
        Augment noise the channels Augment.reverse drops): log p_prior(z | m) + the SplitPriors' log p(half | m) + the forward
        log-det of every inverted layer at its recovered input - log N(dropped Augment channels).  x is the plain call's bit for
        bit.  NotImplementedError for a specialist flow and for a layer without a rule (activation layers, MaskedCoupling).
        differentiable=True: the CONTINUOUS point of the walk - a flow that starts with a Dequantization stops in front of it: the
        tensor floor() would be applied to - and, when grad mode is on and z requires a gradient, with a grad_fn whose backward
        returns dL/dz (a data-only walk: no parameter gradient is formed; once differentiable).  The forward values may differ from
        the plain walk's in rounding.  A specialist flow takes its context and `noise` here too: the codes are formed once, in the
        walk, the couplings run as one cf_flow_step_inv_ctx launch each, and no gradient with respect to a code or the context is
        formed.  The transformer flows: a Conv1x1 -> ActNorm -> TransCoupling step in the one-kernel geometry (smap) is
        walked by the plain walk's launches - there the forward value IS the plain walk's, bit for bit - and its backward is one
        cf_vit_inv_step_bwd_data launch; a context-free TransCoupling anywhere else (msl, smd, atm, fused = False) takes a layer rule
        built from the training backward's kernels.  NotImplementedError with return_logp, with a context for a flow without context
        nets, and for a layer without a rule (a TransCoupling with a context net, MaskedCoupling, a context Coupling outside the fused
        geometry, the activation and spline layers, an Augment over another axis)."""
        if differentiable:
            self._refuse_differentiable("inverse", context, False, return_logp)
            return self._run_differentiable(z, None, context, noise)
        self._refuse_logp(return_logp)
        self._need_context("inverse", context)
        with self._pinned(noise, context):
            return _inv._inverse(self, z, context, None, return_logp=return_logp)

    def _refuse_logp(self, return_logp):
        if return_logp and self._has_context_nets():
            raise NotImplementedError("return_logp: a context-conditioned (specialist) flow - its inverse kernels have no log-det output")

    def sample(self, n_samples, context=None, labels=None, temperature=1.0, noise=None, return_logp=False):
        """flowsequential.py:32-39: a prior draw through the reverse chain.  By specification, for the image flows: the pixels
        are projected into [0, bins - 1].  The reverse chain ends in floor(bins (sigmoid(y) - a) / (1 - 2 a)) (dequantize.py:19-20,
        normalize.py:36-40), which is -1 / bins wherever sigmoid(y) leaves [a, 1 - a) - logits no forward pass can produce, but
        a prior draw does (1.2 % of the pixels of an untrained cifar10 flow) - and a cast of such an image to uint8 wraps -1
        to 255.  The reference's categorical dequantisers clamp their reverse the same way (dequantize.py:67); `inverse` stays
        the plain chain, bitwise.
        labels (an int, or one class index per sample) / temperature: the prior and every SplitPrior on the way back draw
        from the class-mixture of each sample's label, with the components' scales multiplied by `temperature` - one
        cf_gmm_draw launch per level (GaussianMixtureDistribution.draw).  labels=None is class-mixture 1, as the default
        call.  Mixture priors only: ValueError otherwise.
        A specialist flow takes its `context` ((n, nctx) integers; ValueError without one or with another number of rows) and
        draws, by specification, from the density `log_prob(., context)` scores: the prior and every SplitPrior draw from the
        mixtures with the per-sample shifts of their context nets (one cf_gmm_ctx_draw launch per level), where the
        reference's own `sample` ignores the shifts.  noise (`context_noise`): the codes of the stochastic context encoders.
        return_logp: (x, logp) as `inverse` - logp (n, M) is the MODEL's density, the one `log_prob` scores, for every class column
        m, whatever labels and temperature the draw used (no density of the tempered proposal); where a pixel is clamped into
        the data range, logp is still the density of the unclamped continuous point the walk passed through.  x and the random
        numbers consumed are those of the call without the flag."""
        self._refuse_logp(return_logp)
        self._need_context("sample", context)
        if context is not None and self._has_context_nets():
            if not isinstance(self.dist, GaussianMixtureDistribution):
                raise ValueError("sample under a context needs a mixture prior, not %s" % type(self.dist).__name__)
            if context.shape[0] != n_samples:
                raise ValueError("sample: a context of %d rows for %d samples" % (context.shape[0], n_samples))
            with self._pinned(noise, context):
                labels = self.dist._class_labels(labels, n_samples)
                z = self.dist.draw(n_samples, labels, temperature, context=context)
                return _inv._inverse(self, z, context, _inv._pixel_range(self), labels=labels, temperature=temperature, ctx_draw=True)
        if labels is not None or temperature != 1.0:
            if not isinstance(self.dist, GaussianMixtureDistribution):
                raise ValueError("sample: labels / temperature need a mixture prior, not %s" % type(self.dist).__name__)
            labels = self.dist._class_labels(labels, n_samples)      # checked and moved to the device once, for every level
            z = self.dist.draw(n_samples, labels, temperature)
        else:
            z = self.dist.sample(n_samples, context, need_log_prob=False)[0] if isinstance(self.dist, GaussianMixtureDistribution) \
                else self.dist.sample(n_samples, context)[0]       # (the reference's sample() also returns log p(z): the walk scores z itself)
        return _inv._inverse(self, z, context, _inv._pixel_range(self), labels=labels, temperature=temperature, return_logp=return_logp)

    def _split_priors(self):
        return [m for m in self.sequence_modules if isinstance(m, SplitPrior)]

    def encode(self, x, context=None, noise=None):
        """(latents, logp): the complete latent of x - latents = [half_1, ..., half_n, z], the channel half every SplitPrior
        split off, in forward order, and the final z, each a fresh contiguous tensor - and the (B, M) log-densities.  The
        same kernels as `forward` (the fused plan when it applies; never a replayed graph): the halves are the slices the
        mixture kernels score, copied out, and under the same seed / injected noise z and logp are `forward`'s bit for bit.
        `decode` is the way back.
        A specialist flow takes its `context` (ValueError without) and runs layer by layer; noise (`context_noise`): the codes
        of its stochastic context encoders - the same object given to `decode` makes the pair a round trip, and logp is what
        `forward` returns under that noise."""
        _hip.require_device(x)
        self._need_context("encode", context)
        self._refresh_generation()
        halves = []
        with torch.no_grad(), self._pinned(noise, context):
            if self._fusable():
                z, logp = self._forward_fused(x, context, halves=halves)
            else:
                z, logp = self._forward_layers(x, context, halves=halves)
            assert len(halves) == len(self._split_priors())
            latents = [h.clone(memory_format=torch.contiguous_format) for h in halves + [z]]
        return latents, logp

    def decode(self, latents, context=None, clamp=False, noise=None, return_logp=False, differentiable=False):
        """The reverse chain on a complete latent (`encode`'s list: one half per SplitPrior in forward order, then z): every
        SplitPrior puts its half back instead of drawing one.  clamp=True: the projection into the pixel range that `sample`
        applies.  ValueError for a wrong number of latents or a latent whose shape is not its level's.  A specialist flow takes
        its `context` (ValueError without) and `noise` as `encode`.  return_logp: (x, logp) as `inverse` - the halves given
        here are the ones scored; with clamp=True logp stays the density of the unclamped continuous point.
        differentiable=True: as `inverse` - the continuous point, and backward returns the gradient with respect to z and to every
        half that requires one, each in the layout of its latent; the conv flows, the specialist conv flows and the transformer
        flows (smap: one launch per step in the backward; msl / smd / atm: a layer rule).  ValueError together with clamp=True."""
        if differentiable:
            self._refuse_differentiable("decode", context, clamp, return_logp)
        self._refuse_logp(return_logp)
        self._need_context("decode", context)
        latents = list(latents)
        n = len(self._split_priors())
        if len(latents) != n + 1:
            raise ValueError("decode: %d latents for a flow with %d SplitPriors (%d expected: the halves, then z)" % (len(latents), n, n + 1))
        z = latents[-1]
        if any(h.shape[0] != z.shape[0] for h in latents):
            raise ValueError("decode: latents of different batch sizes %s" % [h.shape[0] for h in latents])
        if isinstance(self.dist, GaussianMixtureDistribution) and tuple(z.shape[1:]) != tuple(self.dist.mG.shape[2:]):
            raise ValueError("decode: z of shape %s, the prior is over %s" % (tuple(z.shape), tuple(self.dist.mG.shape[2:])))
        if differentiable:
            return self._run_differentiable(z, latents[:-1], context, noise)
        with self._pinned(noise, context):
            return _inv._inverse(self, z, context, _inv._pixel_range(self) if clamp else None, latents=latents[:-1], return_logp=return_logp)


class FlowInvSequential(nn.Module):
    """Sampling-direction flow of the variational context encoders (flowsequential.py:42-68): draw from `dist`, push
    the sample through the layers' forward, subtract their log-dets from the log-density."""

    def __init__(self, dist, *modules):
        super().__init__()
        self.dist = dist
        for i, module in enumerate(modules):
            self.add_module(str(i), module)
        self.sequence_modules = modules

    def __iter__(self):
        yield from self.sequence_modules

    def forward(self, input, context=None):
        return self.sample(input, context)

    def log_prob(self, input, context=None):
        raise RuntimeError("InverseFlow does not support log_prob, see Flow instead.")

    def sample(self, input, context=None):
        with torch.no_grad():
            output, logprob = self.dist.sample(input.size(0), context)
            for module in self.sequence_modules:
                output, ldj = module(output, context)
                logprob = logprob - ldj
        return output, logprob
