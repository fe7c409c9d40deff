"""Measurements of the defect contours (csrc/contours.hip, uaps_amd/contours.py), DESIGN.md section 3.29.

Shapes 16 x 256 x 256 and 2 x 1024 x 1024 at C = 4, 8-connectivity, M = 256, on the labels of label_instances over the four fillings
of the component bench (tools/bench_components.py's mask builders) and one more
  sparse   about 10 blobs per image, the realistic case
  noise    class noise at density 0.5: about one edge a pixel, far more components than rows, most labels above M
  one      one component filling every image: four turns, one ring of 2 (H + W) edges
  rings    about 10 annuli per image with salt and pepper
  spiral   a one-pixel-wide spiral filling every image: one ring of about H * W edges, every doubling round does work
  classes  the noise mask's class map itself as the label image (three disconnected labels, none above M): about 1.5 edges a
           pixel, the densest input -- what label_instances' 256 rows hide in `noise`
Each is timed as
  call         events around each of `reps` calls of contours() -- trace, the host read of the totals, write -- median and minimum
  launches     per kernel name the median microseconds of a launch, the launches a call and their sum a call (torch.profiler's
               kernel records, in a run of their own; null where it reports none)
  rounds       the pointer-doubling rounds that did work, of those launched
  host         the only route a user has without this feature: the device-to-host copy of the labels, then the numpy tracer of
               uaps_amd/contours.py per image on 16 threads
The device output is asserted equal to the package's CPU path on every input.  Nothing gates on these times.

    python tools/bench_contours.py [--reps 50] [--out profiles/contours_bench.json]

Prints one JSON object."""
import argparse
import json
import math
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
from bench_instances import call_us  # noqa: E402

M = 256
SHAPES = ((16, 256, 256), (2, 1024, 1024))


def spiral(B, H, W):
    """Class 1 on a one-pixel-wide spiral with one-pixel gaps, from the top left corner inwards."""
    m = [[0] * W for _ in range(H)]
    step = ((0, 1), (1, 0), (0, -1), (-1, 0))
    y = x = d = stuck = 0
    m[0][0] = 1
    while stuck < 2:
        dy, dx = step[d]
        y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= y1 < H and 0 <= x1 < W and m[y1][x1] == 0 and (not (0 <= y2 < H and 0 <= x2 < W) or m[y2][x2] == 0):
            y, x, stuck = y1, x1, 0
            m[y][x] = 1
        else:
            d, stuck = (d + 1) % 4, stuck + 1
    return np.repeat(np.array(m, dtype=np.int64)[None], B, axis=0)


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
            if "contour_" in e.name and e.device_time > 0:
                name = e.name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                per.setdefault(name, []).append(e.device_time)
        return {k: {"median_us": statistics.median(v), "launches_per_call": len(v) / reps, "sum_us_per_call": sum(v) / reps}
                for k, v in sorted(per.items())} or None
    except Exception as e:                      # the profiler is a convenience of this tool, not of the product
        return {"error": repr(e)}


def host_today(labels_dev, pool):
    from uaps_amd.contours import _trace_image
    t0 = time.perf_counter()
    labels = labels_dev.cpu().numpy()
    t1 = time.perf_counter()
    list(pool.map(lambda b: _trace_image(labels[b], M, True), range(labels.shape[0])))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uaps_amd import contours, label_instances
    from uaps_amd.contours import _contours_cpu
    dev = torch.device("cuda:0")
    res = {"classes": 4, "connectivity": 8, "max_instances": M, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "host_threads": 16, "cases": []}
    with ThreadPoolExecutor(16) as pool:
        for B, H, W in SHAPES:
            masks = dict(fillings(B, H, W))
            masks["spiral"] = spiral(B, H, W)
            masks["classes"] = masks["noise"]
            for fname, m in masks.items():
                inst = label_instances(torch.from_numpy(m).to(dev), max_instances=M)
                if fname == "classes":
                    inst = inst._replace(labels=torch.from_numpy(m).to(dev).to(torch.int32))
                fn = lambda: contours(inst)
                out = fn()
                ref = _contours_cpu(inst.labels.cpu().numpy(), M, 8)
                for got, want in zip(out[:4], ref[:4]):
                    assert np.array_equal(got.cpu().numpy(), want), (B, H, W, fname)
                us = call_us(fn, a.reps)
                case = {"shape": [B, H, W], "filling": fname, "components_max": int(inst.count.max()),
                        "rings": int(out.rings.shape[0]), "points": int(out.points.shape[0]), "edges": int(out.rings[:, 5].sum()),
                        "longest_ring_edges": int(out.rings[:, 5].max()), "rounds_that_ran": out.rounds,
                        "rounds_launched": max(1, math.ceil(math.log2(4 * H * W))),
                        "workspace_mib": (48 * 4 * B * H * W + 4 * B * (H + 1) * (W + 1)) / 2 ** 20,
                        "call_us_median": statistics.median(us), "call_us_min": min(us), "launches": kernel_us(fn, 10)}
                host = [host_today(inst.labels, pool) for _ in range(3)]
                case["host_copy_us_median"] = statistics.median(h[0] for h in host)
                case["host_numpy_tracer_us_median"] = statistics.median(h[1] for h in host)
                case["speedup_vs_host"] = (case["host_copy_us_median"] + case["host_numpy_tracer_us_median"]) / case["call_us_median"]
                res["cases"].append(case)
                print(B, H, W, fname, case["call_us_median"], case["rounds_that_ran"], case["host_numpy_tracer_us_median"], file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
