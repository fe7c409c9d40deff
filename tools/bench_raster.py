"""Measurements of the polygon rasterisation (csrc/raster.hip, uaps_amd/raster.py), DESIGN.md section 3.32.

Shapes 16 x 256 x 256 and 2 x 1024 x 1024 at C = 4, 8-connectivity, M = 256, on the rings of contours() over the labels of
label_instances over the four fillings of the component bench (tools/bench_components.py's mask builders)
  sparse   about 10 blobs per image, the realistic case
  noise    class noise at density 0.5: far more components than rows, 256 labels of a few pixels each
  full     one component filling every image: one box of the whole frame
  rings    about 10 annuli per image with salt and pepper
each traced and simplified at epsilon 2, and one 4096-row frame (1 x 4096 x 512, stripes four pixels wide: 128 edges of 4096 rows)
through the default edge cut, with every edge on the lane form and with every edge on the wave form.  Each is timed as
  call         events around each of `reps` calls of rasterize_contours(res, reference=True) -- plan, the host read of the
               total, fill -- median and minimum
  launches     per kernel name the median microseconds of a launch, the launches a call and their sum a call (torch.profiler's
               kernel records, in a run of their own; null where it reports none)
  contours     the same events around the contours() call that produced the rings
  host         the only route a user has without this feature: the device-to-host copy of the rings and the reference labels, then
               the numpy path of uaps_amd/raster.py per image on 16 threads
The device output is asserted equal to the package's CPU path on every input.  Nothing gates on these times.

    python tools/bench_raster.py [--reps 30] [--out profiles/raster_bench.json]

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
from bench_instances import call_us  # noqa: E402

M = 256
SHAPES = ((16, 256, 256), (2, 1024, 1024))
TALL = (1, 4096, 512)


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
            if "raster_" in e.name and e.device_time > 0:
                name = e.name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                per.setdefault(name, []).append(e.device_time)
        return {k: {"median_us": statistics.median(v), "launches_per_call": len(v) / reps, "sum_us_per_call": sum(v) / reps}
                for k, v in sorted(per.items())} or None
    except Exception as e:                      # the profiler is a convenience of this tool, not of the product
        return {"error": repr(e)}


def host_today(res, labels_dev, pool):
    """(copy us, numpy us): the rings and the reference to the host, then the package's numpy path an image a thread."""
    from uaps_amd.raster import _raster_cpu
    t0 = time.perf_counter()
    points, offsets, rings, labels = (t.cpu().numpy() for t in (res.points, res.ring_offsets, res.rings, labels_dev))
    t1 = time.perf_counter()
    B, H, W = labels.shape

    def one(b):
        mine = np.nonzero(rings[:, 0] == b)[0]                           # (the rings of an image are consecutive)
        if len(mine) == 0:
            return None
        lo, hi = offsets[mine[0]], offsets[mine[-1] + 1]
        return _raster_cpu(points[lo:hi], offsets[mine[0]:mine[-1] + 2] - lo, np.zeros(len(mine), dtype=np.int64), rings[mine, 1],
                           1, H, W, M, 0, labels[b:b + 1], None, 0)
    list(pool.map(one, range(B)))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6


def measure(res, inst, reps, pool, what, **kw):
    from uaps_amd import rasterize_contours
    fn = lambda: rasterize_contours(res, reference=True, **kw)
    out = fn()
    c = res.contours if hasattr(res, "source") else res
    cpu = rasterize_contours(c._replace(points=c.points.cpu(), ring_offsets=c.ring_offsets.cpu(), rings=c.rings.cpu()),
                             reference=inst.labels.cpu())
    for got, want in ((out.labels, cpu.labels), (out.stats, cpu.stats), (out.overlap, cpu.overlap)):
        assert torch.equal(got.cpu(), want), what
    us = call_us(fn, reps)
    fid = out.fidelity()
    case = {"rings": int(c.rings.shape[0]), "points": int(c.points.shape[0]), "pixels_owned": int(out.stats[..., 0].sum()),
            "overlap": int(out.overlap.sum()), "iou_min": float(np.nanmin(fid["iou"])) if np.isfinite(fid["iou"]).any() else None,
            "call_us_median": statistics.median(us), "call_us_min": min(us), "launches": kernel_us(fn, 10)}
    host = [host_today(c, inst.labels, pool) for _ in range(3)]
    case["host_copy_us_median"] = statistics.median(h[0] for h in host)
    case["host_numpy_us_median"] = statistics.median(h[1] for h in host)
    case["speedup_vs_host"] = (case["host_copy_us_median"] + case["host_numpy_us_median"]) / case["call_us_median"]
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uaps_amd import contours, label_instances, simplify_contours
    dev = torch.device("cuda:0")
    res = {"classes": 4, "connectivity": 8, "max_instances": M, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "host_threads": 16, "epsilon": 2.0, "cases": [], "tall": []}
    with ThreadPoolExecutor(16) as pool:
        for B, H, W in SHAPES:
            masks = fillings(B, H, W)
            for fname, key in (("sparse", "sparse"), ("noise", "noise"), ("full", "one"), ("rings", "rings")):
                inst = label_instances(torch.from_numpy(masks[key]).to(dev), max_instances=M)
                trace = lambda: contours(inst)
                traced = trace()
                trace_us = statistics.median(call_us(trace, a.reps))
                for kind, rs in (("traced", traced), ("epsilon2", simplify_contours(traced, 2.0))):
                    case = {"shape": [B, H, W], "filling": fname, "rings_are": kind, "contours_call_us_median": trace_us}
                    case.update(measure(rs, inst, a.reps, pool, (B, H, W, fname, kind)))
                    res["cases"].append(case)
                    print(B, H, W, fname, kind, case["call_us_median"], case["host_numpy_us_median"], file=sys.stderr, flush=True)
        B, H, W = TALL
        stripes = np.zeros((B, H, W), dtype=np.int64)
        stripes[:, :, (np.arange(W) // 4) % 2 == 0] = 1
        inst = label_instances(torch.from_numpy(stripes).to(dev), max_instances=M)
        traced = contours(inst)
        for form, kw in (("default", {}), ("lane", {"edge_wave_rows": 4096}), ("wave", {"edge_wave_rows": 0})):
            case = {"shape": [B, H, W], "filling": "stripes", "edge_form": form}
            case.update(measure(traced, inst, a.reps, pool, ("tall", form), **kw))
            res["tall"].append(case)
            print(B, H, W, form, case["call_us_median"], file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
