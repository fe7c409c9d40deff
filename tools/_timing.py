"""Timing helpers of the sibling trainers' measurement tools (bench_mean_teacher.py, bench_cct_dct.py, bench_cps.py)."""
import time

import torch


def _timed(fn, reps):
    """Mean ms per call of `fn`, event-to-event over `reps` calls behind one warm-up call."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _kernel_ms(fn, reps):
    """Mean time of the main kernel of the entry point `fn` calls (events on its dispatch)."""
    from uaps_amd import _lib
    fn()
    timers = []
    for _ in range(reps):
        with _lib.LaunchTimer() as t:
            fn()
        timers.append(t)
    torch.cuda.synchronize()
    assert all(t.dispatch for t in timers)
    return sum(t.elapsed_ms() for t in timers) / reps


def _step_ms(tr, data, steps, warmup, unlabelled=True):
    """Wall-clock ms per `tr.train_step` over `steps` steps behind `warmup` steps; `unlabelled=False`: train_step(x_l, y_l) only."""
    def step():
        xl, yl, xu = data.next()
        tr.train_step(xl, yl, xu) if unlabelled else tr.train_step(xl, yl)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps
