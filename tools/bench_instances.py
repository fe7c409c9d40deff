"""Measurements of the defect instance extraction (csrc/instances.hip, uaps_amd/instances.py) at the workload's shape, 16 x 256 x 256,
C = 4, two maps, 8-connectivity, max_instances = 256, on three fillings:
  sparse   about 10 blobs per image, the realistic case
  one      one component covering the image: every atomic of an image goes to one root / one table row
  noise    class noise at density 0.5: the most components (about 20,000 per image; the table overflows, labels and count do not)

Per filling: the median microseconds of one label_instances call (events around each call), the achieved rate on the call's algorithmic
bytes (mask, two maps, labels, count, table, each once), the median microseconds of each of its launches (torch.profiler's kernel
records; null where the profiler reports none), and what a user does today on the same masks: the device-to-host copy, then per image
and class scipy.ndimage.label, find_objects and ndimage.mean of both maps, the images spread over 16 threads.

    python tools/bench_instances.py [--reps 50] [--out profiles/instances_bench.json]

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

from _timing import _timed  # noqa: E402

B, H, W, C, M = 16, 256, 256, 4, 256


def fillings():
    rng = np.random.default_rng(0)
    sparse = np.zeros((B, H, W), dtype=np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        for _ in range(10):
            cy, cx, ry, rx = rng.integers(0, H), rng.integers(0, W), rng.integers(3, 24), rng.integers(3, 24)
            sparse[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = rng.integers(1, C)
    one = np.ones((B, H, W), dtype=np.int64)
    noise = np.where(rng.random((B, H, W)) < 0.5, rng.integers(1, C, (B, H, W)), 0).astype(np.int64)
    return {"sparse": sparse, "one": one, "noise": noise}


def call_us(fn, reps):
    """Per-call times in microseconds, events around every call."""
    fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


def launch_us(fn, reps):
    """Median microseconds per kernel name over `reps` calls, or None where the profiler reports no kernel."""
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
            if "kernel" in e.name and e.device_time > 0 and not e.name.startswith("void at::"):
                name = e.name.replace("(anonymous namespace)::", "").replace("void ", "")
                per.setdefault(name.split("(")[0].split("<")[0], []).append(e.device_time)
        return {k: {"median_us": statistics.median(v), "launches_per_call": len(v) / reps} for k, v in sorted(per.items())} or None
    except Exception as e:                      # the profiler is a convenience of this tool, not of the product
        return {"error": repr(e)}


def host_today(mask_dev, maps_dev, pool):
    """What the package's user does without this feature: copy, then scipy per image and class."""
    from scipy import ndimage
    s8 = np.ones((3, 3), dtype=int)
    t0 = time.perf_counter()
    mask, maps = mask_dev.cpu().numpy(), [v.cpu().numpy() for v in maps_dev]
    t1 = time.perf_counter()

    def image(b):
        n_all = 0
        for c in range(1, C):
            lab, n = ndimage.label(mask[b] == c, structure=s8)
            if n:
                ndimage.find_objects(lab)
                idx = np.arange(1, n + 1)
                for v in maps:
                    ndimage.mean(v[b], lab, idx)
            n_all += n
        return n_all
    comps = sum(pool.map(image, range(B)))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6, comps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uaps_amd import label_instances
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    maps = [torch.rand(B, H, W, device=dev), torch.randn(B, H, W, device=dev)]
    nbytes = B * H * W * (8.0 + 4.0 + 4.0 + 4.0) + B * (4.0 + 72.0 * M)
    res = {"batch": B, "H": H, "W": W, "classes": C, "max_instances": M, "connectivity": 8, "maps": 2, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "algorithmic_bytes": nbytes, "host_threads": 16, "fillings": {}}
    with ThreadPoolExecutor(16) as pool:
        for name, m in fillings().items():
            mask = torch.from_numpy(m).to(dev)
            fn = lambda: label_instances(mask, maps, connectivity=8, max_instances=M)
            r = fn()
            us = call_us(fn, a.reps)
            med = statistics.median(us)
            host = [host_today(mask, maps, pool) for _ in range(5)]
            res["fillings"][name] = {
                "components_per_image": float(r.count.float().mean()), "call_us_median": med, "call_us_min": min(us), "call_us_max": max(us),
                "back_to_back_us": _timed(fn, a.reps) * 1e3, "GB_s": nbytes / (med * 1e-6) / 1e9, "launches": launch_us(fn, 10),
                "host_copy_us_median": statistics.median(h[0] for h in host), "host_scipy_us_median": statistics.median(h[1] for h in host),
                "host_components": host[0][2]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
