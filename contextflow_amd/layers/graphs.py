"""HIP graphs of a FlowSequential: the captured forward, the captured training step and the policy by which `forward` captures and
replays on its own - functions of the flow, which keeps their state (`auto_graph`, `_graphs`, `_graph_policy`, `AUTO_GRAPH_*`)."""
import torch

from . import _hip, coupling as _cpl

AUTO_GRAPH_AFTER = 2             # FlowSequential carries both as class attributes: set them there, on the class or an instance
AUTO_GRAPH_MAX_BATCH = 4096


def _auto_graph(flow, x):
    """Graph replay for small, repeated evaluation batches (the reference's operating point is B = 256, config.py:10:
    ~20 launches of a few microseconds of work each).  Conditions: same shape / dtype / device as the previous calls,
    parameters unchanged since (version counters), in-kernel noise (no injected test noise), no event probes, not
    already capturing.  Anything else runs eagerly, and a parameter update drops the graph."""
    if (not flow.auto_graph or flow.step_events is not None or _cpl.VIT_EVENTS is not None or x.dim() != 4 or x.shape[0] == 0
            or x.shape[0] > flow.AUTO_GRAPH_MAX_BATCH or torch.cuda.is_current_stream_capturing()):
        return None
    for m in flow.sequence_modules:
        d = getattr(m, "dist", None) or getattr(m, "distribution", None)
        if d is not None and getattr(d, "fixed_noise", None) is not None:
            return None
    gkey = (tuple(x.shape), x.dtype, x.device)
    ver = flow._versions()
    st = flow._graphs.get(gkey)
    if st is None or st[1] != ver:
        if len(flow._graphs) >= 8:                   # bounded: each graph owns its intermediates
            flow._graphs.clear()
        flow._graphs[gkey] = [1, ver, None]
        return None
    if st[2] is None:
        if flow._graph_policy.get(gkey) is False:    # measured before for this shape: eager launches are faster
            return None
        st[0] += 1
        if st[0] <= flow.AUTO_GRAPH_AFTER:
            return None
        st[2] = GraphedFlow(flow, x, warmup=1)
        if gkey not in flow._graph_policy:
            flow._graph_policy[gkey] = _replay_wins(flow, st[2], x)
            if not flow._graph_policy[gkey]:
                st[2] = None
                return None
    return st[2]


def _replay_wins(flow, g, x, n=5, rounds=2, margin=0.97):
    """A replayed node costs ~7-12 us whatever its kernel does, eager launches are queued ahead of the running kernel:
    with kernels longer than that (the transformer steps: ~30 us each at a batch of 256) the eager forward can be the
    faster one.  Measured once per input shape (the answer does not depend on parameter values; invalidate_caches()
    forgets it): n eager forwards against n replays between HIP events on the launch stream, best of `rounds` each -
    device time, so that a busy host core (bench.py's CPU-baseline threads) cannot pin the verdict - and the graph is
    only rejected when eager is faster by more than 3 %.  The generator is handed back as it was, so the noise
    sequence does not see the probe."""
    dev = x.device
    gen = torch.cuda.default_generators[dev.index]
    gstate = gen.get_state()
    stream = torch.cuda.current_stream(dev)
    best = []
    for run in (lambda: flow._forward_fused(x, None), lambda: g(x)):
        run()
        t = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(n):
                run()
            e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        best.append(min(t))
    gen.set_state(gstate)
    return best[1] * margin < best[0]


class GraphedFlow:
    """A FlowSequential forward captured once into a HIP graph (launch-bound regime: small batches, where the ~45
    kernel launches + side-stream hand-offs of a call cost more than the kernels).  Replays write into static
    output buffers; the noise layers keep drawing fresh noise (graph-safe Philox offsets)."""

    def __init__(self, flow, example, warmup=2):
        _hip.require_device(example)
        if not flow._fusable():
            raise RuntimeError("capture needs initialised ActNorms (run one forward first) and the fused plan")
        self.flow = flow
        self.static_in = example.detach().clone()
        with torch.no_grad():
            s = torch.cuda.Stream(device=example.device)
            s.wait_stream(torch.cuda.current_stream(example.device))
            gen = torch.cuda.default_generators[example.device.index]
            gstate = gen.get_state()                   # the warm-up passes draw noise positions nobody sees: hand the
            with torch.cuda.stream(s):                 # generator back as it was, so that capturing is invisible in the
                for _ in range(warmup):               # noise sequence (same seed => same noise, captured or not)
                    flow._forward_fused(self.static_in, None)       # warm-up off the default stream: first-use attribute
            torch.cuda.current_stream(example.device).wait_stream(s)   # calls, allocator pools, plan construction
            gen.set_state(gstate)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.static_z, self.static_logp = flow._forward_fused(self.static_in, None)

    def __call__(self, x):
        self.static_in.copy_(x)
        self.graph.replay()
        return self.static_z, self.static_logp


class GraphedTrainStep:
    """See FlowSequential.capture_train_step.

    First call: `warmup` (default 1) EAGER training steps on the given batch - real optimizer updates, off the default
    stream - then the capture of one more step (a capture records, it does not execute: no update).  It returns the loss
    of the last eager step, so with the default warmup the first call is exactly one update, like every later call.
    Later calls replay.  Before the capture and before every replay the optimizer's `push_hyperparameters()` is called if it
    has one: `optim.FusedAdamW` keeps the learning rate in a device scalar that the captured update reads, so a loop that
    assigns floats to `param_group['lr']` between calls (the reference's `warmup_lr`, `scheduler.step()` of `StepLR`) drives the
    captured step unchanged, and `FusedAdamW(max_grad_norm=...)` puts the reference's `clip_grad_norm_` between backward and
    update.  `torch.optim.AdamW(capturable=True)` with a float `lr` stays FROZEN at the rate of the capture - the float is
    baked into its captured launches and later assignments are silently ignored.
    A replay changes the parameters on the device without moving their version counters, which the evaluation caches of
    the flow key on (packed step tables, mixture tables, auto-captured forward graphs): every call therefore ends with
    `flow.invalidate_caches()`, and a `log_prob` between training steps sees the current parameters."""

    def __init__(self, flow, example, loss_fn, optimizer, warmup=1, loss_args=()):
        _hip.require_device(example)
        if not flow._fusable() and not flow._specialist():
            raise RuntimeError("capture_train_step needs initialised ActNorms: run one forward first")
        if warmup < 1:
            raise ValueError("capture_train_step: warmup must be >= 1 (the first call returns the loss of its last eager step)")
        self.flow, self.loss_fn, self.opt = flow, loss_fn, optimizer
        self.static_in = example.detach().clone()
        self.static_args = None
        self.graph = None
        self.warmup = warmup
        self.updates = 0             # optimizer updates performed through this object

    @staticmethod
    def _drain_collectives(dev):
        """Before a capture that contains RCCL collectives: let the process group's watchdog thread retire the EAGER
        collectives of the warm-up step.  It polls their completion events (hipEventQuery) every 100 ms; once the capture has
        pulled RCCL's internal stream into capture mode, HIP answers such a query with hipErrorCapturedEvent ("event last
        recorded in a capturing stream" - for an event recorded BEFORE the capture, on a stream that is capturing NOW), and
        the watchdog aborts the process.  Seen once in four captures with a warm-up step right in front.  The device is idle
        after the synchronize, so every pending work is complete and the next poll (or the one after) drops it."""
        import time
        import torch.distributed as tdist
        if tdist.is_available() and tdist.is_initialized() and tdist.get_backend() == "nccl":
            torch.cuda.synchronize(dev)
            time.sleep(0.35)

    def _push(self):
        # an optimizer that keeps hyper-parameters on the device (optim.FusedAdamW: the learning rate) refreshes them from
        # param_groups here, outside the graph: the captured launches read them from there
        push = getattr(self.opt, "push_hyperparameters", None)
        if push is not None:
            push()

    def _step(self):
        # grads start as None: the autograd engine then TAKES the gradient buffers the backward returns (allocated from
        # the graph's private pool during capture, so their addresses are the ones every replay writes and the
        # optimizer's captured kernels read) instead of a fill + an accumulate launch per parameter
        self.opt.zero_grad(set_to_none=True)
        logp = self.flow.log_prob(self.static_in)
        loss = self.loss_fn(logp, *self.static_args)
        loss.backward()
        self.opt.step()
        return loss

    def __call__(self, x, *loss_args):
        if getattr(self.opt, "_in_ema_scope", False):
            raise RuntimeError("GraphedTrainStep inside the optimizer's ema_scope(): the parameters hold the averages; leave the scope first")
        if self.graph is None:
            self.static_args = tuple(a.detach().clone() if torch.is_tensor(a) else a for a in loss_args)
            self.static_in.copy_(x)
            dev = self.static_in.device
            self._push()
            s = torch.cuda.Stream(device=dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):                   # warm-up steps are real optimizer steps
                for _ in range(self.warmup):
                    first = self._step().detach().clone()
            torch.cuda.current_stream(dev).wait_stream(s)
            self.updates += self.warmup
            if self.flow.data_parallel:
                self._drain_collectives(dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.static_loss = self._step()
            self.flow.invalidate_caches()
            return first
        self.static_in.copy_(x)
        for dst, src in zip(self.static_args, loss_args):
            if torch.is_tensor(dst):
                dst.copy_(src)
        self._push()
        self.graph.replay()
        self.updates += 1
        self.flow.invalidate_caches()
        return self.static_loss
