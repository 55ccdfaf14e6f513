"""AdamW for the flows' many small parameter tensors: torch.optim.AdamW's update in ceil(n / 72) launches.

The reference trains with `optim.AdamW(filter(requires_grad, model.parameters()), lr=...)` (model.py:289) and calls
`optimizer.step()` after every backward (experiment_cl.py:136, experiment_ad.py:213).  A flow has 135 (cifar10) ... 571 (smap)
parameter tensors of 9 ... 147 K elements; torch's fused multi-tensor kernel spends 4 ... 16 launches of 15 - 43 us on them, 12 - 15 % of
the captured training step at the reference's batch of 256.  `FusedAdamW` is a drop-in `torch.optim.Optimizer` whose `step()`
is one `cf_adamw_step_batch` call per parameter group (the tensor table travels in the kernel arguments): same arithmetic term by
term (decoupled weight decay, lerp form of the first moment, bias corrections; amsgrad off), same `state_dict` layout
(`step`, `exp_avg`, `exp_avg_sq` per parameter - the moments are views of ONE flat buffer per group), capturable (the update
count lives on the device).  fp32 parameters on one GPU per group; anything else raises.

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
"""
import ctypes

import torch

from .layers import _hip


def _check_lr(lr):
    if torch.is_tensor(lr):
        raise TypeError("FusedAdamW: lr must be a Python float (got a tensor): assign floats to param_group['lr'] - "
                        "push_hyperparameters() carries them to the device, also for a captured step")
    return float(lr)


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
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, maximize=False, max_grad_norm=None):
        lr = _check_lr(lr)
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
        return (m, v, step)

    def load_state_dict(self, state_dict):
        """torch puts the loaded moments into fresh tensors: copy them back into the flat buffers the kernel updates."""
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
                    for k in ("exp_avg", "exp_avg_sq"):
                        if k in new and new[k] is not views[p][k]:
                            views[p][k].copy_(new[k])
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
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for group, flat, slot in zip(self.param_groups, self._flats, self._lr_dev):
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
            work.append((group, flat, slot, ps, gs))
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
        for group, flat, slot, ps, gs in work:
            flat[2].add_(1.0)                                    # the update count of THIS step, on the device (capturable)
            n = len(ps)
            numel = (ctypes.c_int64 * n)(*[p.numel() for p in ps])
            A = _hip.ptr_array
            beta1, beta2 = group["betas"]
            lr = _check_lr(group["lr"])
            ms, vs = [self.state[p]["exp_avg"] for p in ps], [self.state[p]["exp_avg_sq"] for p in ps]
            if capturing or rec is not None:
                # rate from the device scalar.  Under capture a fill would be baked into the graph: the scalar must be current
                if capturing and lr != slot[1]:
                    raise RuntimeError("FusedAdamW: param_group['lr'] changed since the last push_hyperparameters(); call it "
                                       "before capturing a step (capture_train_step does)")
                _hip.call("cf_adamw_step_batch_dev", n, A(ps), A(gs), A(ms), A(vs), ctypes.cast(numel, ctypes.c_void_p), _hip.p(flat[2]),
                          _hip.p(slot[0]), _hip.p(rec), float(beta1), float(beta2), float(group["eps"]),
                          float(group["weight_decay"]), int(group["maximize"]), _hip.stream())
            else:
                _hip.call("cf_adamw_step_batch", n, A(ps), A(gs), A(ms), A(vs), ctypes.cast(numel, ctypes.c_void_p), _hip.p(flat[2]),
                          lr, float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]),
                          int(group["maximize"]), _hip.stream())
            # the kernel wrote through raw pointers: tell torch, so that everything keyed on `_version` (layers/_derived.py, the
            # auto-captured evaluation graphs) sees the update.  Host-only, also under capture; ONE call for the list (571 single
            # calls cost 0.5 ms of host time for the smap flow, the list 45 us).  The moment views share the counter of their flat buffer
            torch.autograd.graph.increment_version(ps)
            torch.autograd.graph.increment_version((flat[0], flat[1]))
        return loss
