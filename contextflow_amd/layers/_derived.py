"""The one cache of everything derived from parameter VALUES: packed step tables, inverse matrices, log-determinants,
mixture tables - kept by the object that owns them while the tensors they derive from are unchanged.

Entries live in `owner.__dict__["_derived"]`: slot -> (key, value, event).  `key(tensors, ...)` is the version counter and the
storage of every source tensor, so in-place updates and `.to()` miss; writes through `.data` move neither and need
`FlowSequential.invalidate_caches()`, which calls `drop` on every owner.

One rule for every entry:
  * hit: the current stream waits on the event recorded behind the launches that built the value (a later call may run on
    another stream than the one that packed the tables);
  * miss: `build()` runs on the current stream, an event is recorded behind it, the entry replaces the slot's previous one;
  * the current stream is capturing: `build()` runs, nothing is looked up and nothing is stored.  A capturing stream must not
    wait on an event recorded outside the capture, and what is built DURING a capture lives in the graph's private pool with
    events that belong to the capture: it must not outlive it as a cache entry (a later eager call would wait on a captured
    event and read buffers that only exist after a replay)."""
import torch


def key(tensors, *extra):
    return tuple((t._version, t.data_ptr()) for t in tensors) + extra


def get(owner, slot, key, build, dev):
    """The value of `slot` (a string, or a tuple such as ("inv_ws", id(layer))) on `owner` for this key; `build()` makes it, with
    launches on the current stream of `dev` only."""
    host = torch.device(dev).type == "cpu"       # a table of host tensors (component_cdf of a module not moved yet): no streams
    if not host and torch.cuda.is_current_stream_capturing():
        return build()
    entries = owner.__dict__.get("_derived")
    if entries is None:
        entries = owner.__dict__["_derived"] = {}
    hit = entries.get(slot)
    stream = None if host else torch.cuda.current_stream(dev)
    if hit is not None and hit[0] == key:
        if not host:
            stream.wait_event(hit[2])
        return hit[1]
    value = build()
    ev = None
    if not host:
        ev = torch.cuda.Event()
        ev.record(stream)
    entries[slot] = (key, value, ev)
    return value


def drop(owner):
    owner.__dict__.pop("_derived", None)
