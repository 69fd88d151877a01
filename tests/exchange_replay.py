"""Replay rendezvous: W > 1 data-parallel operations on ONE device, in one process and one thread, with no process group.

A data-parallel operation of rank r is a deterministic sequence of exchange-hook calls j = 0 .. J-1 whose (n, flags) are the
same on every rank.  Let R[j] be the rank sum of exchange j.  Pass k = 0, 1, .. runs the whole operation once per rank, every
run from the same start state; the hook

- overwrites the buffer of every call j < k with R[j] (already known),
- records the rank's buffer at call j = k,
- leaves the calls j > k alone: the rest of that run computes on un-reduced data and is discarded.

After the W runs of pass k, R[k] is the float32 sum of the recorded buffers in rank order.  The first pass in which no call is
left to record IS the W-rank operation on every rank: each run of it saw the reduced data at every exchange.  (J + 1) * W runs.

What the harness itself proves on whichever library runs (each a ReplayError, never a retry):
- every run of every pass makes the (n, flags) call sequence of the first run;
- in pass k a rank's buffer at every call j < k holds, before it is overwritten, the bytes the same rank held at the same call
  one pass earlier: the operation is deterministic and the start state complete.

The sum runs left to right in rank order: for W = 2 what any all-reduce gives bit for bit, for W > 2 one valid all-reduce.
The hook never fails a run (a failed exchange would leave the engine's step half open): what goes wrong inside it is kept and
raised after the run.  Nothing here waits on anything: an in-order or deferred exchange is a copy enqueued on the engine's
stream (the MWW_EXCHANGE_IN_ORDER contract itself - everything a deferred bucket needs is enqueued before its hook call), the
flush does nothing, and one device synchronisation follows the W runs of a pass."""
import contextlib
import ctypes

import numpy as np
import torch

from microwakeword_amd import native, parallel


class ReplayError(AssertionError):
    pass


class Exchanges:
    """What replay() saw: ``calls`` - the (n, flags) of every hook call of one run, the flush included; ``reduced`` - R[j] of
    every exchange as float32 arrays; ``runs`` - how often the operation ran; ``passes``."""

    def __init__(self, calls, reduced, runs, passes):
        self.calls, self.reduced, self.runs, self.passes = calls, reduced, runs, passes

    def __len__(self):
        return len(self.reduced)


class Memory:
    """The two forms of the exchanged buffers behind one set of functions: host memory of an emulated library, HBM of the
    GPU library (zero-copy views, every access enqueued on the engine's stream)."""

    def __init__(self, engine):
        self.host = bool(getattr(engine.nl, "host_emulated", False))
        self.device = None if self.host else torch.device("cuda", engine.device)
        self.stream = None
        if not self.host:
            h = engine.device_ptr(native.BUF_STREAM)
            self.stream = torch.cuda.ExternalStream(h, device=self.device) if h else None

    def on_stream(self):
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def view(self, ptr, n):
        if self.host:
            return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * n).from_address(ptr)))
        return parallel.wrap_device_floats(ptr, n, self.device)

    def record(self, view):
        if self.host:
            return view.clone()
        out = torch.empty(view.shape, dtype=view.dtype, device=self.device)   # allocated off the engine's stream, kept past the pass
        with self.on_stream():
            out.copy_(view)
        return out

    def overwrite(self, view, value):
        with self.on_stream():
            view.copy_(value)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def replay(W, make_rank, script, sync_bn=True, reduce_grads=True, close=True, max_exchanges=512):
    """Runs ``script(engine, r)`` as rank r of W for every r, as often as the method needs, and returns
    ``([script's result of rank r in the final pass], Exchanges)``.

    ``make_rank(r)`` returns an engine in its start state (a fresh context, or one reset completely); the harness installs the
    exchange hook (world W, ``sync_bn``, ``reduce_grads``) and, with ``close``, closes the engine after its run.  ``script`` is
    any sequence of library calls; it must read what it returns before it returns (the engine does not outlive the run).
    A script that takes a third argument is told whether its run can still be the final pass's (False: the run's results are
    discarded, expensive reads and checks of its own may be skipped; the library calls must not depend on it)."""
    import inspect
    wants_final = len(inspect.signature(script).parameters) >= 3
    reduced, seq0, runs = [], None, 0
    before = [None] * W   # before[r][j]: what rank r held at call j in the pass before, ahead of the overwrite
    while True:
        k = len(reduced)
        if k > max_exchanges:
            raise ReplayError("more than %d exchanges" % max_exchanges)
        held, results, on_gpu = [], [], False
        for r in range(W):
            eng = make_rank(r)
            mem = Memory(eng)
            on_gpu = on_gpu or not mem.host
            calls, bufs, errors = [], [], []

            def hook(ptr, n, flags, mem=mem, calls=calls, bufs=bufs, errors=errors):
                try:
                    calls.append((int(n), int(flags)))
                    if flags == native.EXCHANGE_FLUSH:
                        return
                    j = len(calls) - 1 - sum(1 for _, f in calls[:-1] if f == native.EXCHANGE_FLUSH)
                    if j > k:   # past call k: nothing more is recorded or overwritten in this run
                        return
                    v = mem.view(ptr, n)
                    bufs.append(mem.record(v))
                    if j < k:
                        mem.overwrite(v, reduced[j])
                except Exception as e:   # never fail the run: the engine's step has to complete
                    errors.append(e)

            eng.set_allreduce_hook(hook, W, sync_bn=sync_bn, reduce_grads=reduce_grads)
            try:
                n_known = None if seq0 is None else sum(1 for _, f in seq0 if f != native.EXCHANGE_FLUSH)
                results.append(script(eng, r, n_known is None or k >= n_known) if wants_final else script(eng, r))
                eng.synchronize()
            finally:
                if close:
                    eng.close()
                else:
                    eng.set_allreduce_hook(None)
            runs += 1
            if errors:
                raise errors[0]
            if seq0 is None:
                seq0 = list(calls)
            if calls != seq0:
                raise ReplayError("pass %d rank %d: hook calls %r differ from the first run's %r" % (k, r, calls, seq0))
            held.append(bufs)
        if on_gpu:
            torch.cuda.synchronize()
        for r in range(W):
            if before[r] is not None:
                for j in range(min(k, len(before[r]))):
                    if not _same_bits(held[r][j], before[r][j]):
                        a, b = held[r][j].cpu().numpy(), before[r][j].cpu().numpy()
                        raise ReplayError("pass %d rank %d exchange %d: %d of %d floats differ from the pass before (worst %.3g): the "
                                          "operation is not deterministic, or its start state not complete"
                                          % (k, r, j, int((a.view(np.int32) != b.view(np.int32)).sum()), a.size, float(np.abs(a - b).max())))
        before = held
        if len(held[0]) <= k:   # nothing left to record: this pass was the W-rank operation
            if any(len(h) != k for h in held):
                raise ReplayError("ranks disagree on the number of exchanges")
            return results, Exchanges(seq0, [t.cpu().numpy().copy() for t in reduced], runs, k + 1)
        total = held[0][k].clone()
        for r in range(1, W):
            total = total + held[r][k]   # float32, left to right in rank order
        reduced.append(total)
        if on_gpu:
            torch.cuda.synchronize()
