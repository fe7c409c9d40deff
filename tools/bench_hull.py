"""Measurements of the convex-hull descriptors (csrc/hull.hip, uaps_amd/hull.py), DESIGN.md section 3.28.

Shapes 16 x 256 x 256 and 2 x 1024 x 1024 at C = 4, 8-connectivity, M = 256, on the labels of label_instances over the four fillings
of the component bench (tools/bench_shapes.py's mask builders)
  sparse   about 10 blobs per image, the realistic case
  noise    class noise at density 0.5: far more components than rows, most labels above M
  one      one component filling every image: the longest chains (H + 1 lattice lines), reduced by one lane each
  rings    about 10 annuli per image with salt and pepper
Each is timed as
  call         events around each of `reps` calls, median and minimum (tools/bench_instances.py: call_us), and the mean of
               back-to-back calls (tools/_timing.py: _timed), which hides the launch gaps an isolated call pays
  launches     the median microseconds of every kernel of the call (torch.profiler's kernel records; null where it reports none),
               and the measure kernel alone by events on its dispatch (tools/_timing.py: _kernel_ms)
  host         the only route a user has without this feature: the device-to-host copy of the labels, then per defect
               scipy.spatial.ConvexHull on the pixel corners and a numpy caliper loop over the hull's edges, on 16 threads
The device table is asserted equal to the package's CPU path on every input.  Nothing gates on these times.

    python tools/bench_hull.py [--reps 50] [--out profiles/hull_bench.json]

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
from bench_shapes import call_us, fillings, launch_us  # noqa: E402

M = 256
SHAPES = ((16, 256, 256), (2, 1024, 1024))


def host_defect(ys, xs):
    """qhull on the pixel corners, then calipers over the hull's edges in float64: area, both Feret diameters, the rectangle."""
    from scipy.spatial import ConvexHull
    corners = np.unique(np.concatenate([np.stack([xs + dx, ys + dy], axis=1) for dy in (0, 1) for dx in (0, 1)]), axis=0).astype(np.float64)
    hull = ConvexHull(corners)
    V = corners[hull.vertices]
    d = V[:, None, :] - V[None, :, :]
    fmax = np.sqrt((d * d).sum(-1).max())
    best_w, best_r = np.inf, np.inf
    for i in range(len(V)):
        e = V[(i + 1) % len(V)] - V[i]
        e = e / np.hypot(e[0], e[1])
        along, across = (V - V[i]) @ e, (V - V[i]) @ np.array([-e[1], e[0]])
        w = np.ptp(across)
        best_w, best_r = min(best_w, w), min(best_r, w * np.ptp(along))
    return hull.volume, fmax, best_w, best_r


def host_today(labels_dev, pool):
    t0 = time.perf_counter()
    labels = labels_dev.cpu().numpy()
    t1 = time.perf_counter()
    jobs = []
    for b in range(labels.shape[0]):
        y, x = np.nonzero((labels[b] >= 1) & (labels[b] <= M))
        k = labels[b][y, x]
        order = np.argsort(k, kind="stable")
        y, x, k = y[order], x[order], k[order]
        cuts = np.flatnonzero(np.diff(k)) + 1
        jobs += list(zip(np.split(y, cuts), np.split(x, cuts)))
    list(pool.map(lambda j: host_defect(*j), [j for j in jobs if len(j[0])]))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6, len(jobs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uaps_amd import hull_descriptors, label_instances
    from uaps_amd.hull import _hull_cpu
    dev = torch.device("cuda:0")
    res = {"classes": 4, "connectivity": 8, "max_instances": M, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "host_threads": 16, "cases": []}
    with ThreadPoolExecutor(16) as pool:
        for B, H, W in SHAPES:
            for fname, m in fillings(B, H, W).items():
                inst = label_instances(torch.from_numpy(m).to(dev), max_instances=M)
                fn = lambda: hull_descriptors(inst)
                table = fn().table
                assert np.array_equal(table.cpu().numpy(), _hull_cpu(inst.labels.cpu().numpy(), M)), (B, H, W, fname)
                us = call_us(fn, a.reps)
                case = {"shape": [B, H, W], "filling": fname, "components_max": int(inst.count.max()),
                        "rows_with_a_pixel": int((table[..., 0] > 0).sum()), "vertices_max": int(table[..., 0].max()),
                        "call_us_median": statistics.median(us), "call_us_min": min(us),
                        "back_to_back_us_mean": _timed(fn, a.reps) * 1e3, "launches": launch_us(fn, 10),
                        "measure_kernel_us_mean": _kernel_ms(fn, 10) * 1e3}
                host = [host_today(inst.labels, pool) for _ in range(3)]
                case["host_copy_us_median"] = statistics.median(h[0] for h in host)
                case["host_qhull_calipers_us_median"] = statistics.median(h[1] for h in host)
                case["host_defects"] = host[0][2]
                case["speedup_vs_host"] = (case["host_copy_us_median"] + case["host_qhull_calipers_us_median"]) / case["call_us_median"]
                res["cases"].append(case)
                print(B, H, W, fname, case["call_us_median"], case["host_qhull_calipers_us_median"], file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
