"""Measurements of the component clean-up (csrc/components.hip, uaps_amd/components.py), DESIGN.md section 3.25.

Shapes 16 x 256 x 256 and 2 x 1024 x 1024 at C = 4, 8-connectivity; chains
  open16            [("area_open", 16)]
  fill              [("fill_holes", None)]
  open16_fill64     [("area_open", 16), ("fill_holes", 64)]
  all               [("clear_border",), ("area_open", 16), ("fill_holes", 64)]
on the three fillings of the instance bench and one with holes
  sparse   about 10 blobs per image, the realistic case
  noise    class noise at density 0.5: the most components
  one      one component filling every image: every atomic of an image goes to one word
  rings    about 10 annuli per image with salt and pepper: what the hole steps are for
Each case is timed as
  call         events around each of `reps` calls, median and minimum; and back to back (event to event over all calls)
  apply        the apply pass of the chain's first step alone (events on its dispatch)
  launches     the median microseconds of every kernel of the call (torch.profiler's kernel records; null where it reports none) and
               their sum per call, "kernels_us_sum": the rate on kernel time is formed on it
  composition  where the parent commit had one on the device: label_instances(mask, min_area=n) followed by
               torch.where(labels > 0, mask, background), for the area opening
  host         the device-to-host copy, then scipy label / bincount / binary_fill_holes per image on 16 threads
Nothing gates on these times.  "algorithmic_bytes" is 16 bytes a pixel (the int64 map read once, written once); "traffic_bytes" is a
MODEL of what the launches move per step over p planes (1, or the class count of a hole step): the map read by the tile pass (8 p),
parent and area words written (8 p), parents read and roots written by the flatten pass (8 p), the map read and written by the apply
pass (16) and its root and area look-ups (at most 8 p).

    python tools/bench_components.py [--reps 50] [--out profiles/components_bench.json]

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

from _timing import _kernel_ms, _timed  # noqa: E402
from bench_instances import call_us, launch_us  # noqa: E402

C = 4
SHAPES = ((16, 256, 256), (2, 1024, 1024))
CHAINS = {"open16": [("area_open", 16)], "fill": [("fill_holes", None)], "open16_fill64": [("area_open", 16), ("fill_holes", 64)],
          "all": [("clear_border",), ("area_open", 16), ("fill_holes", 64)]}


def fillings(B, H, W):
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    sparse = np.zeros((B, H, W), dtype=np.int64)
    rings = np.zeros((B, H, W), dtype=np.int64)
    for b in range(B):
        for _ in range(10):
            cy, cx, ry, rx = rng.integers(0, H), rng.integers(0, W), rng.integers(3, H // 10), rng.integers(3, W // 10)
            sparse[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = rng.integers(1, C)
        for _ in range(10):
            cy, cx, ro = rng.integers(-4, H + 4), rng.integers(-4, W + 4), rng.uniform(6.0, H / 8.0)
            d2 = (yy - cy) ** 2 + (xx - cx) ** 2
            rings[b][(d2 <= ro * ro) & (d2 >= (0.6 * ro) ** 2)] = rng.integers(1, C)
        u = rng.random((H, W))
        rings[b][u < 0.01] = 0
        rings[b][u > 0.99] = rng.integers(1, C, (H, W))[u > 0.99]
    noise = np.where(rng.random((B, H, W)) < 0.5, rng.integers(1, C, (B, H, W)), 0).astype(np.int64)
    return {"sparse": sparse, "noise": noise, "one": np.ones((B, H, W), dtype=np.int64), "rings": rings}


def traffic_bytes(steps, N):
    total = 0.0
    for s in steps:
        p = C - 1 if s[0] == "fill_holes" else 1
        total += N * (8.0 * p + 8.0 * p + 8.0 * p + 16.0 + 8.0 * p)
    return total


def host_today(mask_dev, steps, pool):
    """What the package's user does without this feature: copy, then scipy per image (tests/components_ref.py)."""
    import components_ref
    t0 = time.perf_counter()
    mask = mask_dev.cpu().numpy()
    t1 = time.perf_counter()

    def image(b):
        m = mask[b]
        for s in steps:
            m = components_ref.step_image(m, tuple(s), list(range(1, C)), 0, 8)
        return 0
    list(pool.map(image, range(mask.shape[0])))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))         # the scipy reference of the tests
    from uaps_amd import components, label_instances
    dev = torch.device("cuda:0")
    res = {"classes": C, "connectivity": 8, "reps": a.reps, "device": torch.cuda.get_device_name(0), "bytes_per_pixel": 16,
           "host_threads": 16, "cases": []}
    with ThreadPoolExecutor(16) as pool:
        for B, H, W in SHAPES:
            N = float(B * H * W)
            for fname, m in fillings(B, H, W).items():
                mask = torch.from_numpy(m).to(dev)
                for cname, steps in CHAINS.items():
                    fn = lambda: components(mask, steps, C)
                    out = fn()
                    us = call_us(fn, a.reps)
                    med = statistics.median(us)
                    launches = launch_us(fn, 10)
                    ksum = None
                    if launches and "error" not in launches:
                        ksum = sum(v["median_us"] * v["launches_per_call"] for v in launches.values())
                    case = {"shape": [B, H, W], "filling": fname, "chain": cname, "changed_pixels": int((out != mask).sum()),
                            "call_us_median": med, "call_us_min": min(us), "back_to_back_us": _timed(fn, a.reps) * 1e3,
                            "apply_kernel_us_mean": _kernel_ms(fn, a.reps) * 1e3, "launches": launches, "kernels_us_sum": ksum,
                            "algorithmic_bytes": 16.0 * N, "traffic_bytes": traffic_bytes(steps, N),
                            "GB_s_call_algorithmic": 16.0 * N / (med * 1e-6) / 1e9,
                            "GB_s_kernels_traffic": traffic_bytes(steps, N) / (ksum * 1e-6) / 1e9 if ksum else None}
                    if cname == "open16":
                        def composition():
                            r = label_instances(mask, min_area=16)
                            return torch.where(r.labels > 0, mask, torch.zeros_like(mask))
                        assert torch.equal(composition(), out)
                        case["label_instances_where_us_median"] = statistics.median(call_us(composition, a.reps))
                    host = [host_today(mask, steps, pool) for _ in range(3)]
                    case["host_copy_us_median"] = statistics.median(h[0] for h in host)
                    case["host_scipy_us_median"] = statistics.median(h[1] for h in host)
                    res["cases"].append(case)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
