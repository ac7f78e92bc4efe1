"""The gate harness of tests/test_streams_gpu.py: one library call on a busy non-default stream.

``gated_call(fn, inputs, poison, stream)`` runs ``fn`` three ways:

1. baseline -- twice on the default stream of an idle, synchronised device; the two results must be bit-equal; the host time of the
   second call is ``t_host``.  In the same pass ``fn`` runs on the poison of every gated input (one at a time, or all at once with
   ``joint``) and on every ``controls`` variant: each must give ANOTHER result, or the row would prove nothing;
2. gated -- on a non-blocking stream ``s`` (``side_stream``) the device buffers of the inputs are allocated and the gated ones filled with their
   poison (a valid input of the same shape: a library that reads too early computes a wrong answer, never a wild access).  Then, under
   ``s``: event g0, the gate (a device-side delay of G = max(20 ms, 4 t_host) capped at 500 ms), ``buf.copy_(real)`` for every gated
   input, event g1, and without any synchronisation ``fn(bufs)``.  ``pending = not g1.query()`` on return;
3. read-out -- still on ``s`` every output is cloned by a torch op ordered behind the call, ``s`` is synchronised and the clones must
   equal the baseline bit for bit.

Outputs a wrapper allocates itself cannot be pre-filled by the caller; instead tensors of the outputs' shapes are filled with a
sentinel on ``s`` and freed just before the gate, so that the caching allocator hands the wrapper those very blocks: a result that is
never written, or written late from another stream, then differs from the baseline.

The gate is ``torch.cuda._sleep`` with cycles per millisecond from one event-timed call per process, or a chain of matmuls if the
sleep kernel does not behave.  A row is valid only if the gate was still pending when the call returned; for the entries the header
documents as not waiting for the stream that is asserted (``never_waits``), which is also the test of that sentence.
"""
import math
import time

import torch

DEV = "cuda:0"
G_MIN_MS, G_MAX_MS = 20.0, 500.0
SENTINEL_F, SENTINEL_I = -777.25, -7


class _GateState:
    mode = None          # "sleep" | "matmul"
    rate = 0.0           # sleep: cycles per ms; matmul: ms per matmul
    a = c = None


_G = _GateState()
ROWS_SEEN = []           # (entry, t_host ms, G ms, pending): what the run printed, for the summary test
SCENARIO_T_MS = 100.0    # t_host of the multi-call scenarios: G = 400 ms, several calls and a gc.collect() fit in front of it
_STREAMS = {}


class quiet_gc:
    """``with quiet_gc():`` -- a ``gc.collect()`` inside the block looks at objects made inside it only (everything older is
    frozen).  At the end of a long test session a full collection walks the whole heap and outlasts any gate."""

    def __enter__(self):
        import gc
        gc.collect()
        gc.freeze()

    def __exit__(self, *exc):
        import gc
        gc.unfreeze()


def side_stream(i, dev=DEV):
    """Non-blocking stream 0 or 1 of this process, made once: with the default stream that is three streams, fewer than the four
    hardware queues a process gets (torch hands every ``torch.cuda.Stream()`` another of its 32 pooled streams)."""
    assert i in (0, 1)
    if i not in _STREAMS:
        _STREAMS[i] = torch.cuda.Stream(dev)
    return _STREAMS[i]


def _timed_ms(enqueue):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    enqueue()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate(dev=DEV):
    """Once per process, on the default stream of a synchronised device."""
    if _G.mode is not None:
        return _G
    torch.cuda.synchronize(dev)
    with torch.cuda.device(dev):
        try:
            torch.cuda._sleep(1000)                  # loads the kernel
            torch.cuda.synchronize(dev)
            n = 2_000_000
            ms = _timed_ms(lambda: torch.cuda._sleep(n))
            rate = n / ms if ms > 0 else 0.0
            check = _timed_ms(lambda: torch.cuda._sleep(int(20.0 * rate))) if rate > 0 else 0.0
            if 0.02 <= ms <= 5000.0 and 10.0 <= check <= 40.0:
                _G.mode, _G.rate = "sleep", rate
        except (AttributeError, RuntimeError):
            pass
        if _G.mode is None:
            _G.a = torch.full((2048, 2048), 1.0 / 2048, device=dev)
            _G.c = torch.empty_like(_G.a)
            torch.mm(_G.a, _G.a, out=_G.c)
            torch.cuda.synchronize(dev)
            ms = _timed_ms(lambda: [torch.mm(_G.a, _G.a, out=_G.c) for _ in range(20)]) / 20
            _G.mode, _G.rate = "matmul", max(ms, 1e-3)
    print(f"stream gate: {_G.mode}, {_G.rate:.4g} {'cycles per ms' if _G.mode == 'sleep' else 'ms per matmul'}")
    return _G


def gate(ms):
    """Enqueue a delay of ``ms`` milliseconds on the current stream."""
    calibrate()
    if _G.mode == "sleep":
        torch.cuda._sleep(int(ms * _G.rate))
    else:
        for _ in range(int(math.ceil(ms / _G.rate))):
            torch.mm(_G.a, _G.a, out=_G.c)


def gate_ms(t_host_ms):
    return min(max(G_MIN_MS, 4.0 * t_host_ms), G_MAX_MS)


def flat(out, prefix=""):
    """[(name, tensor)] of whatever a wrapper returns: tensors, None, numbers, and tuples / lists / dicts of them."""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [(prefix or "out", out)]
    if isinstance(out, dict):
        return [x for k in sorted(out) for x in flat(out[k], f"{prefix}.{k}" if prefix else str(k))]
    if isinstance(out, (tuple, list)):
        return [x for i, v in enumerate(out) for x in flat(v, f"{prefix}[{i}]")]
    if isinstance(out, (bool, int, float)):
        return [(prefix or "out", torch.tensor(out))]
    raise TypeError(f"{prefix}: cannot compare a {type(out).__name__}")


def host(out):
    """The outputs as cloned host tensors (a torch copy on the current stream, which it waits for)."""
    return [(n, t.detach().clone().cpu()) for n, t in flat(out)]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.contiguous().numpy().tobytes() == b.contiguous().numpy().tobytes()


def differing(got, want):
    """Names of the outputs that are not bit-equal (or are missing on one side)."""
    if [n for n, _ in got] != [n for n, _ in want]:
        return ["<structure>"]
    return [n for (n, a), (_, b) in zip(got, want) if not same(a, b)]


def baseline(fn, inputs, poison, joint=False, controls=(), dev=DEV, entry=""):
    """-> (host outputs, t_host in ms).  Default stream, idle device; asserts run-to-run equality and that every poison bites."""
    torch.cuda.synchronize(dev)
    real = {k: v.to(dev) for k, v in inputs.items()}
    torch.cuda.synchronize(dev)
    first = host(fn(dict(real)))
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn(dict(real))
    t_host = (time.perf_counter() - t0) * 1e3
    second = host(out)
    assert not differing(first, second), (entry, "two runs on the default stream differ", differing(first, second))
    sets = [tuple(poison)] if joint else [(k,) for k in poison]
    for keys in sets:
        if not keys:
            continue
        bad = dict(real, **{k: poison[k].to(dev) for k in keys})
        assert differing(host(fn(bad)), second), (entry, f"the poison of {keys} changes no output: the row would prove nothing")
    for name, alt in controls:
        assert differing(host(alt(dict(real))), second), (entry, f"control '{name}' changes no output: the row would prove nothing")
    torch.cuda.synchronize(dev)
    return second, t_host


def soil(like, dev=DEV):
    """Sentinel-filled tensors of the outputs' shapes on the current stream, freed at once: what the wrapper's torch.empty gets."""
    for _, t in like:
        if t.numel():
            s = torch.empty(t.shape, dtype=t.dtype, device=dev)
            s.fill_(SENTINEL_F if t.dtype.is_floating_point else (True if t.dtype == torch.bool else SENTINEL_I))
            del s


class Gated:
    """``with Gated(stream, t_host_ms, {buf: real}) as g:`` -- under ``stream``: g0, the gate, the copies, g1; ``g.pending()``."""

    def __init__(self, stream, t_host_ms, copies, dev=DEV):
        self.stream, self.G, self.copies = stream, gate_ms(t_host_ms), copies
        self.g0, self.g1 = torch.cuda.Event(), torch.cuda.Event()
        self._ctx = torch.cuda.stream(stream)

    def __enter__(self):
        self._ctx.__enter__()
        self.g0.record()
        gate(self.G)
        for buf, real in self.copies:
            buf.copy_(real)
        self.g1.record()
        return self

    def pending(self):
        return not self.g1.query()

    def __exit__(self, *exc):
        return self._ctx.__exit__(*exc)


def gated_call(fn, inputs, poison, stream=None, *, entry="", never_waits=False, joint=False, controls=(), after=None, dev=DEV):
    """One row.  ``fn(dict name -> device tensor)`` -> outputs; ``inputs``: name -> host tensor; ``poison``: name -> host tensor for the
    gated inputs (the others are in place before the gate).  ``controls``: (name, fn) variants that must give another result on the
    default stream.  ``after(outputs)``: runs behind the read-out, on the synchronised stream.  -> dict(t_host, G, pending)."""
    calibrate(dev)
    want, t_host = baseline(fn, inputs, poison, joint, controls, dev, entry)
    s = stream if stream is not None else side_stream(0, dev)
    with torch.cuda.stream(s):
        real = {k: v.to(dev) for k, v in inputs.items()}
        bufs = {k: (poison[k].to(dev) if k in poison else real[k]) for k in inputs}
        soil(want, dev)
    s.synchronize()
    with Gated(s, t_host, [(bufs[k], real[k]) for k in poison], dev) as g:
        out = fn(dict(bufs))
        pending = g.pending()
        got = [(n, t.detach().clone()) for n, t in flat(out)]         # ordered behind the call on s
        s.synchronize()
        got = [(n, t.cpu()) for n, t in got]
    ROWS_SEEN.append((entry, t_host, g.G, pending))
    print(f"{entry:44s} t_host {t_host:8.3f} ms  G {g.G:6.1f} ms  pending={pending}")
    bad = differing(got, want)
    assert not bad, (entry, "outputs differ from the default-stream baseline", bad)
    if never_waits:
        assert pending, (entry, f"the call returned after the gate ({g.G:.0f} ms): it waited for the stream, or the host spent "
                                f"more than four times its idle-device time ({t_host:.2f} ms) in it")
    if after is not None:
        after(out)
    return dict(t_host=t_host, G=g.G, pending=pending)
