"""AdamW for the flows' many small parameter tensors: torch.optim.AdamW's update in ceil(n / 72) launches, optionally with an
exponential moving average of the parameters written by the same kernel (ceil(n / 64) launches then).

The reference trains with `optim.AdamW(filter(requires_grad, model.parameters()), lr=...)` (model.py:289) and calls
`optimizer.step()` after every backward (experiment_cl.py:136, experiment_ad.py:213).  A flow has 135 (cifar10) ... 571 (smap)
parameter tensors of 9 ... 147 K elements; torch's fused multi-tensor kernel spends 4 ... 16 launches of 15 - 43 us on them, 12 - 15 % of
the captured training step at the reference's batch of 256.  `FusedAdamW` is a drop-in `torch.optim.Optimizer` whose `step()`
is one `cf_adamw_step_batch` call per parameter group (the tensor table travels in the kernel arguments): same arithmetic term by
term (decoupled weight decay, lerp form of the first moment, bias corrections; amsgrad off), same `state_dict` layout
(`step`, `exp_avg`, `exp_avg_sq` per parameter - the moments are views of ONE flat buffer per group; with `ema_decay` one more
entry, `ema`), capturable (the update count lives on the device).  fp32 parameters on one GPU per group; anything else raises.

Schedules and clipping (the reference's `warmup_lr`, experiment_cl.py:98-105 / experiment_ad.py:175-181, `StepLR`, model.py:290,
and `clip_grad_norm_`, experiment_cl.py:135 / experiment_ad.py:212).  Each group's learning rate also lives in a one-element fp64
device scalar that `push_hyperparameters()` fills from `group["lr"]`; a `step()` under stream capture reads the rate from there
(`cf_adamw_step_batch_dev`), so a captured step follows whatever floats the training loop assigns to `param_group["lr"]` -
`GraphedTrainStep` pushes before the capture and before every replay.  `max_grad_norm=X` fuses `clip_grad_norm_(all parameters,
X)` into the step: `cf_grad_norm_batch` (fp64 sum of squares in a fixed order, then the norm and torch's clipping coefficient on
the device) and the update multiplies every gradient element by the coefficient in a register - `p.grad` itself stays
UNSCALED, unlike after `clip_grad_norm_`.  A non-finite gradient makes the norm non-finite and the coefficient 0 or NaN, exactly
as torch's `clip_grad_norm_(error_if_nonfinite=False)` followed by `step()`: there is no skip-step policy.
Which kernel a `step()` launches: without `max_grad_norm`, the host-rate form (`cf_adamw_step_batch`) in eager mode and the
device-rate form under capture.  With `max_grad_norm`, ALWAYS the device-rate form, eager included, because the fused scale exists
only there; such an eager `step()` calls `push_hyperparameters()` itself first.  The two forms give the same bits for the same
rate (`test_device_learning_rate_equals_host_learning_rate`).
`clip_grad_norm_` below is the eager drop-in for the reference's line, on the same kernels.

What torch sees of a step.  The kernels write parameters and moments through raw pointers, so `step()` advances the `_version`
counter of every tensor it wrote (the parameters that had a gradient, their `exp_avg` and `exp_avg_sq`) itself, in both kernel
forms, eager and under capture: everything keyed on the counters - the parameter-derived tables of layers/_derived.py, the
auto-captured evaluation graphs - follows an eager training loop as it follows torch.optim.AdamW.  The REPLAY of a captured step
runs no Python and moves no counter: `GraphedTrainStep` calls `invalidate_caches()` after every replay for that reason.

The update count.  `state[p]["step"]` of every parameter of a group is a view of ONE device scalar per group, advanced once per
`step()` in which at least one parameter of the group had a gradient.  A parameter that sits a step out (`grad is None`) keeps its
parameter and moments but its bias corrections use the group's count from then on - torch.optim.AdamW counts per parameter.  The
flows here give every trainable parameter a gradient in every step, where the two agree.  `load_state_dict` takes the count of the
group's last parameter that carries one.  The moments are allocated at construction for the parameters that require a gradient
then: a parameter unfrozen later has none, and `step()` raises instead of skipping or guessing - build a new optimizer.

The average (`ema_decay=d`, Polyak / EMA weights; off by default, and then every call runs the code it ran without it).  Each group
gets one more flat buffer laid out like the moments, `state[p]["ema"]` a view shaped like `p`, FILLED WITH THE PARAMETERS' VALUES AT
CONSTRUCTION.  The update kernel (`cf_adamw_ema_step_batch` / `..._dev`, in whichever of the three forms `step()` would have chosen)
writes, in the thread that just updated the parameter element, `ema = p` at the group's update count t = 1 and
`ema += w (p - ema)`, `w = (float)(1 - d_t)`, afterwards; `d_t = min(d, (1 + t) / (10 + t))` with `ema_warmup=True`, else `d`, formed
in double on the device from the count the kernel reads for the bias corrections.  So the average needs no kernel of its own and no host work (ceil(n / 64) update launches per group instead of ceil(n / 72)),
and a REPLAYED captured step advances it and follows the warm-up of the decay.  Parameters, moments and count are bit for bit
those of the same run without the average.  Like the bias corrections, the average goes by the group's SHARED count: a parameter
that sits update 1 out keeps its construction copy (no element is ever uninitialised) and lerps from it at its first own update;
the count's t = 1 copy happens only for the parameters that had a gradient in that step.  `ema_parameters()` returns the averages,
`ema_scope(flow)` evaluates under them.  Data-parallel training needs nothing more: every rank applies the same averaged gradient to
the same parameters, so the ranks' averages agree bit for bit as their parameters do.  Buffers (the ActNorm `initialized` flags) are
not averaged; a non-finite gradient poisons parameters and average alike.
"""
import contextlib
import ctypes

import torch

from .layers import _hip


def _check_lr(lr):
    if torch.is_tensor(lr):
        raise TypeError("FusedAdamW: lr must be a Python float (got a tensor): assign floats to param_group['lr'] - "
                        "push_hyperparameters() carries them to the device, also for a captured step")
    return float(lr)


def _check_ema(ema_decay, ema_warmup):
    if ema_decay is None:
        if ema_warmup:
            raise ValueError("FusedAdamW: ema_warmup needs ema_decay")
        return None
    if torch.is_tensor(ema_decay) or isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 <= ema_decay < 1.0:
        raise ValueError("FusedAdamW: ema_decay must be a Python float in [0, 1) or None (got %r)" % (ema_decay,))
    return float(ema_decay)


def _grad_table(grads):
    """(n, host array of device pointers, host array of element counts) of a list of contiguous fp32 gradients"""
    n = len(grads)
    numel = (ctypes.c_int64 * n)(*[g.numel() for g in grads])
    return n, (_hip.ptr_array(grads) if n else ctypes.c_void_p(0)), numel


def _norm_partials(numels):
    """Number of fp64 partials cf_grad_norm_batch writes for these element counts (host-only query)."""
    n = len(numels)
    arr = (ctypes.c_int64 * max(n, 1))(*numels)
    got = int(_hip.lib().cf_grad_norm_partials(n, ctypes.cast(arr, ctypes.c_void_p)))
    if got < 0:
        raise ValueError("cf_grad_norm_partials: bad element counts %r" % (list(numels),))
    return got


class _NormWorkspace:
    """fp64 partials + the {norm, coef} record of the norm kernels, allocated once per (owner, device) and grown only when the
    parameter set does: a captured step sees fixed addresses."""

    def __init__(self, device, partials):
        self.partials = torch.empty(max(partials, 1), device=device, dtype=torch.float64)
        self.rec = torch.zeros(2, device=device, dtype=torch.float32)

    def run(self, grads, max_norm):
        n, ptrs, numel = _grad_table(grads)
        _hip.call("cf_grad_norm_batch", n, ptrs, ctypes.cast(numel, ctypes.c_void_p), float(max_norm), _hip.p(self.partials),
                  self.partials.numel(), _hip.p(self.rec), _hip.stream())


def _checked_grads(params):
    gs = []
    for p in params:
        g = p.grad
        if g.is_sparse or g.dtype != torch.float32 or not g.is_cuda:
            raise RuntimeError("clip_grad_norm_: dense fp32 gradients on a GPU")
        if gs and g.device != gs[0].device:
            raise RuntimeError("clip_grad_norm_: gradients on one GPU (got %s and %s)" % (gs[0].device, g.device))
        gs.append(g)
    return gs


# device -> _NormWorkspace of the standalone clip_grad_norm_.  ONE per device, shared by every caller: calls for one device must
# be ordered on ONE stream (two streams would race on the partials and the record).  It is replaced by a larger one when a larger
# gradient set appears (the returned norms are clones, so earlier results stay valid); under capture that would move addresses a
# graph holds, so there it raises.
_CLIP_WS = {}


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """`torch.nn.utils.clip_grad_norm_(parameters, max_norm)` (experiment_cl.py:135, experiment_ad.py:212) in ceil(n / 224) + 1
    launches for the norm and ceil(n / 224) for the in-place scale, whatever the number of tensors: the gradients are
    multiplied by min(1, max_norm / (norm + 1e-6)) and the norm BEFORE clipping is returned as a 0-dim device tensor (no
    host sync).  The norm is accumulated in fp64.  Only the 2-norm; non-finite gradients behave as with torch's
    error_if_nonfinite=False.  The workspace is one per device: issue all calls for a device on one stream."""
    if float(norm_type) != 2.0:
        raise ValueError("clip_grad_norm_: only norm_type=2 is implemented (got %r)" % (norm_type,))
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError("clip_grad_norm_: max_norm must be > 0 (got %r)" % (max_norm,))
    if torch.is_tensor(parameters):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return torch.zeros(())
    gs = _checked_grads(params)
    for g in gs:
        if not g.is_contiguous():
            raise RuntimeError("clip_grad_norm_: gradients must be contiguous (they are scaled in place)")
    dev = gs[0].device
    need = _norm_partials([g.numel() for g in gs])
    ws = _CLIP_WS.get(dev)
    if ws is None or ws.partials.numel() < need:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("clip_grad_norm_: first call for this gradient set under capture; call it once eagerly first")
        ws = _CLIP_WS[dev] = _NormWorkspace(dev, need)
    with torch.no_grad():
        ws.run(gs, max_norm)
        n, ptrs, numel = _grad_table(gs)
        _hip.call("cf_grad_scale_batch", n, ptrs, ctypes.cast(numel, ctypes.c_void_p), _hip.p(ws.rec), _hip.stream())
        return ws.rec[0].clone()


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, maximize=False, max_grad_norm=None,
                 ema_decay=None, ema_warmup=False):
        lr = _check_lr(lr)
        self.ema_decay = _check_ema(ema_decay, ema_warmup)
        self.ema_warmup = bool(ema_warmup)
        self._ema_flats = []         # per parameter group: the flat buffer of the averages | None (ema_decay)
        self._in_ema_scope = False   # ema_scope(): the parameters hold the averages - no update, no replay, no second entry
        if max_grad_norm is not None:
            if torch.is_tensor(max_grad_norm) or not float(max_grad_norm) > 0.0:
                raise ValueError("FusedAdamW: max_grad_norm must be a float > 0 or None (got %r)" % (max_grad_norm,))
            max_grad_norm = float(max_grad_norm)
        self.max_grad_norm = max_grad_norm
        self._lr_dev = []            # per parameter group: [fp64 device scalar | None, the float it holds]
        self._norm_ws = None         # _NormWorkspace over every parameter of every group (max_grad_norm)
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not 0.0 <= weight_decay:
            raise ValueError("FusedAdamW: invalid hyper-parameters lr=%r betas=%r eps=%r weight_decay=%r" % (lr, betas, eps, weight_decay))
        self._flats = []             # per parameter group: (exp_avg flat, exp_avg_sq flat, step) | None - kept out of param_groups
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, maximize=bool(maximize)))

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        self._flats.append(self._init_group(group))
        flat = self._flats[-1]
        lr = _check_lr(group["lr"])
        # the rate on the device, for the captured form of the step (push_hyperparameters keeps it current)
        self._lr_dev.append([None, None] if flat is None else [torch.full((1,), lr, device=flat[2].device, dtype=torch.float64), lr])
        self._norm_ws = None

    def _init_group(self, group):
        ps = [p for p in group["params"] if p.requires_grad]
        if not ps:
            self._ema_flats.append(None)
            return None
        dev = ps[0].device
        for p in ps:
            if p.dtype != torch.float32 or p.device != dev or not p.is_cuda:
                raise RuntimeError("FusedAdamW: fp32 parameters on one GPU per group (got %s on %s)" % (p.dtype, p.device))
            if not p.is_contiguous():
                raise RuntimeError("FusedAdamW: parameters must be contiguous")
        offs, o = [], 0
        for p in ps:
            offs.append(o)
            o += (p.numel() + 3) & ~3                            # 16-byte aligned slots: the kernel moves float4s
        m = torch.zeros(max(o, 1), device=dev, dtype=torch.float32)
        v = torch.zeros_like(m)
        step = torch.zeros(1, device=dev, dtype=torch.float32)
        for p, lo in zip(ps, offs):
            self.state[p] = {"step": step[0], "exp_avg": m[lo:lo + p.numel()].view_as(p), "exp_avg_sq": v[lo:lo + p.numel()].view_as(p)}
        ema = None
        if self.ema_decay is not None:
            # the average starts as a copy of the parameters: a parameter that sits the first update out lerps from this copy later
            ema = torch.zeros_like(m)
            for p, lo in zip(ps, offs):
                self.state[p]["ema"] = ema[lo:lo + p.numel()].view_as(p)
            self._fill_ema(ps)
        self._ema_flats.append(ema)
        return (m, v, step)

    def _fill_ema(self, ps):
        with torch.no_grad():
            torch._foreach_copy_([self.state[p]["ema"] for p in ps], [p.detach() for p in ps])

    def load_state_dict(self, state_dict):
        """torch puts the loaded moments into fresh tensors: copy them back into the flat buffers the kernel updates.  The `ema`
        entry travels the same way.  A dict WITHOUT `ema` (saved by an optimizer without `ema_decay`) is no error: the average of
        such a parameter is re-filled from the CURRENT parameter values, as at construction.  A dict with `ema` loaded into an
        optimizer without `ema_decay` drops the entry."""
        views = {p: dict(self.state[p]) for g in self.param_groups for p in g["params"] if p in self.state}
        super().load_state_dict(state_dict)
        for g, flat in zip(self.param_groups, self._flats):
            if flat is None:
                continue
            loaded_step = None
            for p in g["params"]:
                if p not in views:
                    continue
                new = self.state.get(p, {})
                with torch.no_grad():
                    for k in ("exp_avg", "exp_avg_sq", "ema"):
                        if k in views[p] and k in new and new[k] is not views[p][k]:
                            views[p][k].copy_(new[k])
                    if "ema" in views[p] and "ema" not in new:
                        views[p]["ema"].copy_(p.detach())
                    if "step" in new:
                        loaded_step = float(new["step"])
                self.state[p] = views[p]
            if loaded_step is not None:
                flat[2].fill_(loaded_step)

    def push_hyperparameters(self):
        """Carry each group's `lr` (a Python float, as `warmup_lr` / `StepLR` assign it) to the device scalar the captured
        form of `step()` reads: one asynchronous fill per group whose value changed since the last push, no host sync.
        Call it before capturing a step and before every replay (`GraphedTrainStep` does)."""
        for group, slot in zip(self.param_groups, self._lr_dev):
            if slot[0] is None:
                continue
            lr = _check_lr(group["lr"])
            if not 0.0 <= lr:
                raise ValueError("FusedAdamW: invalid lr=%r" % (lr,))
            if lr != slot[1]:
                slot[0].fill_(lr)
                slot[1] = lr

    @property
    def grad_norm(self):
        """Global gradient 2-norm of the last step (before clipping): a 0-dim view of the device record the next step - or
        replay - overwrites; reading it does not sync.  None without `max_grad_norm` or before the first step."""
        return None if self._norm_ws is None else self._norm_ws.rec[0]

    def _workspace(self, dev):
        if self._norm_ws is None:
            numels = [p.numel() for g in self.param_groups for p in g["params"] if p.requires_grad]
            self._norm_ws = _NormWorkspace(dev, _norm_partials(numels))
        elif self._norm_ws.rec.device != dev:
            raise RuntimeError("FusedAdamW(max_grad_norm): every parameter group on one GPU (the norm is global)")
        return self._norm_ws

    @torch.no_grad()
    def step(self, closure=None):
        if self._in_ema_scope:
            raise RuntimeError("FusedAdamW.step() inside ema_scope(): the parameters hold the averages; leave the scope first")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for group, flat, slot, ema in zip(self.param_groups, self._flats, self._lr_dev, self._ema_flats):
            ps = [p for p in group["params"] if p.requires_grad and p.grad is not None]
            if not ps:
                continue
            gs = []
            for p in ps:
                if flat is None or "exp_avg" not in self.state.get(p, ()):
                    raise RuntimeError("FusedAdamW: a parameter of shape %s has a gradient but no moments - it did not require a gradient "
                                       "when the optimizer was built.  The moments are allocated at construction (one flat buffer per "
                                       "group): build a new FusedAdamW after unfreezing parameters" % (tuple(p.shape),))
                g = p.grad
                if g.is_sparse or g.dtype != torch.float32 or g.device != p.device:
                    raise RuntimeError("FusedAdamW: dense fp32 gradients on the parameter's device")
                gs.append(g if g.is_contiguous() else g.contiguous())
            work.append((group, flat, slot, ps, gs, ema))
        if not work:
            return loss
        capturing = torch.cuda.is_current_stream_capturing()
        rec = None
        if self.max_grad_norm is not None:
            # ONE norm over every gradient of every group, as clip_grad_norm_(model.parameters(), ...) takes it
            # (the fused scale lives in the device-rate kernel only, so this path uses it in eager mode too: make the scalars current)
            if not capturing:
                self.push_hyperparameters()
            ws = self._workspace(work[0][3][0].device)
            ws.run([g for w in work for g in w[4]], self.max_grad_norm)
            rec = ws.rec
        for group, flat, slot, ps, gs, ema in work:
            flat[2].add_(1.0)                                    # the update count of THIS step, on the device (capturable)
            n = len(ps)
            numel = (ctypes.c_int64 * n)(*[p.numel() for p in ps])
            A = _hip.ptr_array
            beta1, beta2 = group["betas"]
            lr = _check_lr(group["lr"])
            ms, vs = [self.state[p]["exp_avg"] for p in ps], [self.state[p]["exp_avg_sq"] for p in ps]
            tail = ()
            if ema is not None:
                es = [self.state[p]["ema"] for p in ps]
                tail = (self.ema_decay, int(self.ema_warmup))
            if capturing or rec is not None:
                # rate from the device scalar.  Under capture a fill would be baked into the graph: the scalar must be current
                if capturing and lr != slot[1]:
                    raise RuntimeError("FusedAdamW: param_group['lr'] changed since the last push_hyperparameters(); call it "
                                       "before capturing a step (capture_train_step does)")
                name, head = (("cf_adamw_step_batch_dev", (A(ps), A(gs), A(ms), A(vs))) if ema is None else
                              ("cf_adamw_ema_step_batch_dev", (A(ps), A(gs), A(ms), A(vs), A(es))))
                _hip.call(name, n, *head, ctypes.cast(numel, ctypes.c_void_p), _hip.p(flat[2]),
                          _hip.p(slot[0]), _hip.p(rec), float(beta1), float(beta2), float(group["eps"]),
                          float(group["weight_decay"]), int(group["maximize"]), *tail, _hip.stream())
            else:
                name, head = (("cf_adamw_step_batch", (A(ps), A(gs), A(ms), A(vs))) if ema is None else
                              ("cf_adamw_ema_step_batch", (A(ps), A(gs), A(ms), A(vs), A(es))))
                _hip.call(name, n, *head, ctypes.cast(numel, ctypes.c_void_p), _hip.p(flat[2]),
                          lr, float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]),
                          int(group["maximize"]), *tail, _hip.stream())
            # the kernel wrote through raw pointers: tell torch, so that everything keyed on `_version` (layers/_derived.py, the
            # auto-captured evaluation graphs) sees the update.  Host-only, also under capture; ONE call for the list (571 single
            # calls cost 0.5 ms of host time for the smap flow, the list 45 us).  The moment views share the counter of their flat buffer
            torch.autograd.graph.increment_version(ps)
            torch.autograd.graph.increment_version((flat[0], flat[1]) if ema is None else (flat[0], flat[1], ema))
        return loss

    def ema_parameters(self):
        """The averages (`state[p]["ema"]`, views of the groups' flat buffers) in `param_groups` order, for the parameters that
        have one (those that required a gradient at construction).  Empty without `ema_decay`."""
        return [self.state[p]["ema"] for g in self.param_groups for p in g["params"] if "ema" in self.state.get(p, ())]

    def _swap_ema(self):
        """Exchange parameters and averages, group by group.  Every group is checked before the first launch, and a launch that
        fails after others went through exchanges those back before the error leaves: all groups swapped, or none."""
        work = []
        for g, ema in zip(self.param_groups, self._ema_flats):
            ps = [p for p in g["params"] if "ema" in self.state.get(p, ())]
            if ema is None or not ps:
                continue
            for p in ps:
                if not p.is_contiguous() or p.dtype != torch.float32 or p.device != ema.device:
                    raise RuntimeError("FusedAdamW.ema_scope: a parameter left the form it had at construction (contiguous fp32 on %s)" % (ema.device,))
            work.append((ps, ema))
        done = []
        try:
            for ps, ema in work:
                self._swap_group(ps, ema)
                done.append((ps, ema))
        except BaseException:
            for ps, ema in done:
                self._swap_group(ps, ema)
            raise

    def _swap_group(self, ps, ema):
        with torch.no_grad():
            numel = (ctypes.c_int64 * len(ps))(*[p.numel() for p in ps])
            _hip.call("cf_swap_batch", len(ps), _hip.ptr_array(ps), _hip.ptr_array([self.state[p]["ema"] for p in ps]),
                      ctypes.cast(numel, ctypes.c_void_p), _hip.stream())
            torch.autograd.graph.increment_version(ps)
            torch.autograd.graph.increment_version((ema,))

    @contextlib.contextmanager
    def ema_scope(self, flow=None):
        """Evaluate under the averaged weights: `with opt.ema_scope(flow): flow.log_prob(x)`.  On entry and on exit ONE
        `cf_swap_batch` per group exchanges the CONTENTS of every parameter with its average - the addresses stay, so a captured
        training graph stays valid - and the version counters of everything written advance.  Inside, `state[p]["ema"]` holds the
        raw iterate.  Give the flow when a captured step (`capture_train_step`) trains it: a replay moves no counter, so the flow's
        evaluation caches may hold tables of either weight set, and `flow.invalidate_caches()` is called on both sides.  The
        parameters are restored on exceptions too.  Not re-entrant; `step()` and a replay of `GraphedTrainStep` raise inside
        the scope, as does `state_dict()`; not under stream capture.  Every rank of a data-parallel run may enter on its own: the averages agree."""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdamW.ema_scope: built without ema_decay")
        if self._in_ema_scope:
            raise RuntimeError("FusedAdamW.ema_scope is not re-entrant")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamW.ema_scope under stream capture: a replay would exchange the weights again")
        self._swap_ema()                                         # all groups or none: nothing to undo when it raises
        self._in_ema_scope = True
        try:
            if flow is not None:
                flow.invalidate_caches()
            yield self
        finally:
            try:
                self._swap_ema()
            finally:
                # all or none again; if the way back failed the parameters still hold the averages, and the error says so by
                # leaving - the flag must not lock the optimizer for good on top of it
                self._in_ema_scope = False
                if flow is not None:
                    flow.invalidate_caches()

    def state_dict(self):
        """torch's layout (+ `ema` per parameter with `ema_decay`).  Inside `ema_scope()` parameters and averages are exchanged, so
        a dict taken there would carry the raw iterate under `ema`: it raises instead."""
        if self._in_ema_scope:
            raise RuntimeError("FusedAdamW.state_dict() inside ema_scope(): parameters and averages are exchanged; leave the scope first")
        return super().state_dict()
