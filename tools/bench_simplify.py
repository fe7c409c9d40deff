"""Measurements of the contour simplification (csrc/simplify.hip, uaps_amd/simplify.py), DESIGN.md section 3.30.

The masks of tools/bench_contours.py (sparse, noise, one, rings, spiral, classes) at 16 x 256 x 256 and 2 x 1024 x 1024, traced by
contours() at 8-connectivity and M = 256, simplified at epsilon 0.75 and 2.  Each is timed as
  call         events around each of `reps` calls of simplify_contours() -- mark, the host read of the total, write -- median and
               minimum, at the default thresholds, with the wave form off (wave_max = 0) and with the wave and the LDS form off
               (wave_max = lds_max = 0: the global form for every ring)
  launches     per kernel name the median microseconds of a launch, the launches a call and their sum a call (torch.profiler's
               kernel records, in a run of their own, default thresholds; null where it reports none)
  points       before and after, and the rings that took each form
  host         the route a user has without this feature: the device-to-host copy of points, offsets, rings and summary, then the
               package's CPU path (numpy, an explicit stack per ring) over chunks of rings on 16 threads
The device output is asserted equal to the package's CPU path on every input.  No counters are collected.  Nothing gates on these
times.

    python tools/bench_simplify.py [--reps 30] [--out profiles/simplify_bench.json]

Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_components import fillings  # noqa: E402
from bench_contours import M, SHAPES, spiral  # noqa: E402
from bench_instances import call_us  # noqa: E402

EPSILONS = (0.75, 2.0)
FORMS = (("default", {}), ("no_wave", {"wave_max": 0}), ("global_only", {"wave_max": 0, "lds_max": 0}))
THREADS = 16


def kernel_us(fn, reps):
    """Per kernel name: the median microseconds of a launch, the launches a call and the sum a call; None without kernel records."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        per = {}
        for e in prof.events():
            if "simplify_" in e.name and e.device_time > 0:
                name = e.name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                per.setdefault(name, []).append(e.device_time)
        return {k: {"median_us": statistics.median(v), "launches_per_call": len(v) / reps, "sum_us_per_call": sum(v) / reps}
                for k, v in sorted(per.items())} or None
    except Exception as e:                      # the profiler is a convenience of this tool, not of the product
        return {"error": repr(e)}


def host_today(res, e16, pool):
    """(copy, simplification) in microseconds: the four arrays to the host, then the CPU path's ring function over chunks of rings."""
    from uaps_amd.simplify import _simplify_ring
    t0 = time.perf_counter()
    points, offsets = res.points.cpu().numpy().astype(np.int64), res.ring_offsets.cpu().numpy()
    res.rings.cpu(), res.summary.cpu()
    t1 = time.perf_counter()
    L = len(offsets) - 1
    bounds = np.linspace(0, L, 4 * THREADS + 1).astype(int)
    work = lambda c: [_simplify_ring(points[offsets[r]:offsets[r + 1]], e16 * e16) for r in range(bounds[c], bounds[c + 1])]
    list(pool.map(work, range(4 * THREADS)))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    from uaps_amd import contours, label_instances, simplify_contours
    from uaps_amd.simplify import _simplify_cpu, quantise
    dev = torch.device("cuda:0")
    out = {"connectivity": 8, "max_instances": M, "reps": a.reps, "device": torch.cuda.get_device_name(0), "host_threads": THREADS,
           "counters": None, "cases": []}
    with ThreadPoolExecutor(THREADS) as pool:
        for B, H, W in SHAPES:
            masks = dict(fillings(B, H, W))
            masks["spiral"] = spiral(B, H, W)
            masks["classes"] = masks["noise"]
            for fname, m in masks.items():
                inst = label_instances(torch.from_numpy(m).to(dev), max_instances=M)
                if fname == "classes":
                    inst = inst._replace(labels=torch.from_numpy(m).to(dev).to(torch.int32))
                res = contours(inst)
                n = res.rings[:, 4]
                for eps in EPSILONS:
                    e16 = quantise(eps)
                    got = simplify_contours(res, eps)
                    ref = _simplify_cpu(res.points.cpu().numpy(), res.ring_offsets.cpu().numpy(), res.rings.cpu().numpy(),
                                        res.summary.cpu().numpy(), e16)
                    for x, y in zip(tuple(got.contours[:4]) + (got.ring_stats,), ref):
                        assert np.array_equal(x.cpu().numpy(), y), (B, H, W, fname, eps)
                    case = {"shape": [B, H, W], "filling": fname, "epsilon": eps, "rings": int(res.rings.shape[0]),
                            "points_before": int(res.points.shape[0]), "points_after": int(got.contours.points.shape[0]),
                            "longest_ring_points": int(n.max()), "rings_wave_form": int((n <= 64).sum()),
                            "rings_lds_form": int(((n > 64) & (n <= 2048)).sum()), "rings_global_form": int((n > 2048).sum())}
                    for name, kw in FORMS:
                        fn = lambda: simplify_contours(res, eps, **kw)
                        alt = fn()
                        assert all(torch.equal(x, y) for x, y in zip(alt.contours[:4], got.contours[:4]))
                        us = call_us(fn, a.reps)
                        case[f"call_us_median_{name}"], case[f"call_us_min_{name}"] = statistics.median(us), min(us)
                    case["launches"] = kernel_us(lambda: simplify_contours(res, eps), 5)
                    host = [host_today(res, e16, pool) for _ in range(a.host_reps)]
                    case["host_copy_us_median"] = statistics.median(h[0] for h in host)
                    case["host_cpu_path_us_median"] = statistics.median(h[1] for h in host)
                    case["speedup_vs_host"] = (case["host_copy_us_median"] + case["host_cpu_path_us_median"]) / case["call_us_median_default"]
                    out["cases"].append(case)
                    print(B, H, W, fname, eps, case["points_before"], case["points_after"], case["call_us_median_default"],
                          case["call_us_median_no_wave"], case["call_us_median_global_only"], case["host_cpu_path_us_median"],
                          file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
