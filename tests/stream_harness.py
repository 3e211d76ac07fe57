"""Helpers of the stream-contract tests (test_stream_contract_gpu.py): a side
stream, a bounded delay on it, inputs that arrive late, and the check that the
stream was still busy when it mattered ("armed").

Everything runs in this process on at most two user streams beside torch's
default one, and nothing runs beside a call under test: the delay sits on the
call's own stream, in front of it.  The delay is finite and on that one stream
-- no host-released gate -- so a call that synchronises inside cannot hang on
it.  Not a test module and not a conftest."""
import ctypes
import time

import torch

from multilinear_amd import device as D

CHAIN_LOG = 22  # the delay's fallback: NTT / INTT pairs of this size

_cal = {}


def side_stream():
    """A fresh torch stream (torch's pool streams are non-blocking): entered
    with ``with torch.cuda.stream(S):`` so that D.context() binds to it."""
    return torch.cuda.Stream()


def _time_on(S, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    S.synchronize()
    a.record(S)
    fn()
    b.record(S)
    b.synchronize()
    return a.elapsed_time(b)


def _chain_pair(S):
    c = _cal["chain"]
    lib, ctx = D.lib(), D.context()
    D.check(lib.mlh_ntt(ctx, D.ptr(c["x"]), D.ptr(c["x"]), CHAIN_LOG, c["g"]), ctx)
    D.check(lib.mlh_intt(ctx, D.ptr(c["x"]), D.ptr(c["x"]), CHAIN_LOG, c["g"]), ctx)


def _calibrate(S):
    """Once per process: how long the delay's unit takes on this device."""
    if "kind" in _cal:
        return
    with torch.cuda.stream(S):
        if hasattr(torch.cuda, "_sleep"):
            cycles = 1000000
            torch.cuda._sleep(cycles)  # (the first launch loads the kernel)
            ms = _time_on(S, lambda: torch.cuda._sleep(cycles))
            if ms > 0.05:  # it really waits: cycles per millisecond
                _cal["kind"], _cal["rate"] = "sleep", cycles / ms
                return
        g = (ctypes.c_uint8 * 16)()
        assert D.lib().mlh_pow_2_generator(CHAIN_LOG, g) == 0
        _cal["chain"] = dict(x=D.random_device(1 << CHAIN_LOG, 4242), g=g)
        _chain_pair(S)  # builds the tables
        _cal["kind"], _cal["rate"] = "chain", 1.0 / max(_time_on(S, lambda: _chain_pair(S)), 1e-3)


def delay(S, ms):
    """Enqueue at least ``ms`` milliseconds of work on S; returns at once."""
    _calibrate(S)
    with torch.cuda.stream(S):
        if _cal["kind"] == "sleep":
            torch.cuda._sleep(int(ms * _cal["rate"] * 1.25) + 1)
        else:
            for _ in range(int(ms * _cal["rate"] * 1.25) + 1):
                _chain_pair(S)


def late_inputs(S, pairs, ms):
    """pairs: [(true_tensor, decoy_tensor)].  -> ([buffers], ready): each
    buffer holds its decoy now and receives its true tensor by a copy enqueued
    on S behind delay(S, ms); ``ready`` is an event recorded on S after the
    copies.  The decoys are canonical data of the same shape, so work that
    reads a buffer out of stream order computes a wrong answer, not a fault."""
    with torch.cuda.stream(S):
        bufs = [decoy.clone() for _, decoy in pairs]
        for (true, decoy), buf in zip(pairs, bufs):
            assert true.shape == decoy.shape and true.dtype == decoy.dtype
            assert not torch.equal(true, decoy)
        S.synchronize()  # the decoys are in place before the delay starts
        delay(S, ms)
        for (true, _), buf in zip(pairs, bufs):
            buf.copy_(true, non_blocking=True)
        ready = torch.cuda.Event()
        ready.record(S)
    return bufs, ready


def late_input(S, true_tensor, decoy_tensor, ms):
    """One buffer of late_inputs -> (buffer, ready)."""
    bufs, ready = late_inputs(S, [(true_tensor, decoy_tensor)], ms)
    return bufs[0], ready


def run_armed(S, name, make_inputs, call, syncs):
    """Run ``call`` twice on S: on the idle stream with the true inputs, then
    with late inputs behind a delay of max(2, 4 x the idle run's host wall
    time) ms.  -> (idle result, armed result); the caller compares both with
    the oracle.

    make_inputs() -> [(true, decoy)] device tensors, the same values every
    time, fresh tensors every time (a call may work in place).
    call(*buffers) -> finish: the call under test on the current stream; a
    call that does not synchronise also enqueues, on the same stream and with
    no host wait, whatever consumes its output (a copy into another tensor).
    finish() is called after S.synchronize() and returns host values.
    syncs: the call returns host results, so it waits for the stream itself.

    Armed: the stream was still busy -- ``ready`` not reached -- right after a
    call that does not synchronise returned, or right before one that does.  A
    run that was not armed is repeated once with twice the delay and fresh
    buffers; if that is not armed either, the test fails."""
    with torch.cuda.stream(S):
        pairs = make_inputs()
        S.synchronize()
        t0 = time.perf_counter()
        finish = call(*[true.clone() for true, _ in pairs])
        S.synchronize()
        idle_ms = (time.perf_counter() - t0) * 1e3
        idle = finish()
        ms = max(2.0, 4.0 * idle_ms)
        for attempt in (0, 1):
            pairs = make_inputs()
            S.synchronize()
            bufs, ready = late_inputs(S, pairs, ms)
            if syncs:
                armed = ready.query() is False
                finish = call(*bufs)
            else:
                finish = call(*bufs)
                armed = ready.query() is False
            S.synchronize()
            got = finish()
            if armed:
                break
            if attempt == 0:
                ms *= 2.0
        print("stream %s: idle call %.3f ms, delay %.1f ms (%s), %s"
              % (name, idle_ms, ms, _cal["kind"], "armed" if armed else "not armed"))
        assert armed, "not armed: %s %s the stream had drained (delay %.1f ms)" % (
            name, "before the call" if syncs else "when the call returned", ms)
    return idle, got


def busy(S, ms):
    """For work that has no device input to deliver late: a delay on S and the
    event behind it.  -> ready."""
    with torch.cuda.stream(S):
        delay(S, ms)
        ready = torch.cuda.Event()
        ready.record(S)
    return ready
