"""Measurements of the boundary metrics (csrc/surface.hip, uaps_amd/surface.py) at 16 x 256 x 256 and 2 x 1024 x 1024, C = 4, int64
label maps, percentile 95, tolerance 2, on three inputs:
  shifted   about 10 blobs per image, the prediction is the target moved by 2 px: masks that nearly agree, the realistic case
  noise     class noise on both sides: almost every pixel is a surface pixel, every scan is short
  far       one block per side in opposite corners: few surface pixels, and every one scans outwards across most of the row

Per input: the median microseconds of one surface_distances call (events around each call), the achieved rate on the call's
algorithmic bytes (both label maps and the table, each once), the median microseconds of each of its launches (torch.profiler's kernel
records; null where the profiler reports none), the same for distance_transform_sq of the prediction's foreground, and what a user does
today on the same masks: the device-to-host copy, then per image and class scipy binary_erosion, distance_transform_edt both ways,
np.percentile and the means, the (image, class) pairs spread over 16 threads.

    python tools/bench_surface.py [--reps 30] [--out profiles/surface_bench.json]

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
from bench_instances import call_us, launch_us  # noqa: E402

C = 4
SIZES = ((16, 256, 256), (2, 1024, 1024))


def inputs(B, H, W):
    rng = np.random.default_rng(0)
    target = np.zeros((B, H, W), dtype=np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        for _ in range(10):
            cy, cx, ry, rx = rng.integers(0, H), rng.integers(0, W), rng.integers(H // 80 + 2, H // 10), rng.integers(W // 80 + 2, W // 10)
            target[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = rng.integers(1, C)
    shifted = np.zeros_like(target)
    shifted[:, 2:, :] = target[:, :-2, :]
    far_p, far_t = np.zeros_like(target), np.zeros_like(target)
    far_p[:, : H // 8, : W // 8] = 1
    far_t[:, -(H // 8):, -(W // 8):] = 1
    return {"shifted": (shifted, target), "noise": (rng.integers(0, C, (B, H, W)), rng.integers(0, C, (B, H, W))), "far": (far_p, far_t)}


def host_today(pred_dev, target_dev, pool):
    """What the package's user does without this feature: copy, then scipy per image and class."""
    from scipy import ndimage
    cross = ndimage.generate_binary_structure(2, 1)
    t0 = time.perf_counter()
    pred, target = pred_dev.cpu().numpy(), target_dev.cpu().numpy()
    t1 = time.perf_counter()

    def pair(bc):
        b, c = bc
        fp, fg = pred[b] == c, target[b] == c
        sp, sg = fp ^ ndimage.binary_erosion(fp, cross), fg ^ ndimage.binary_erosion(fg, cross)
        if not sp.any() or not sg.any():
            return 0
        dp, dg = ndimage.distance_transform_edt(~sg)[sp], ndimage.distance_transform_edt(~sp)[sg]
        np.percentile(np.hstack((dp, dg)), 95)
        (dp.mean() + dg.mean()) / 2
        return 1
    pairs = sum(pool.map(pair, [(b, c) for b in range(pred.shape[0]) for c in range(1, C)]))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uaps_amd import distance_transform_sq, surface_distances
    dev = torch.device("cuda:0")
    res = {"classes": C, "percentile": 95.0, "tolerance": 2.0, "label_dtype": "int64", "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "host_threads": 16, "sizes": {}}
    with ThreadPoolExecutor(16) as pool:
        for B, H, W in SIZES:
            nbytes = B * H * W * 16.0 + B * C * 96.0
            size = res["sizes"][f"{B}x{H}x{W}"] = {"algorithmic_bytes": nbytes, "edt_algorithmic_bytes": B * H * W * 5.0, "inputs": {}}
            for name, (p, t) in inputs(B, H, W).items():
                pred, target = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
                fn = lambda: surface_distances(pred, target, C, tolerance=2.0)
                fg = pred > 0
                edt = lambda: distance_transform_sq(fg)
                s = fn().summary()
                us, eus = call_us(fn, a.reps), call_us(edt, a.reps)
                med, emed = statistics.median(us), statistics.median(eus)
                host = [host_today(pred, target, pool) for _ in range(3)]
                hmed = statistics.median(h[0] + h[1] for h in host)
                size["inputs"][name] = {
                    "summary": s, "call_us_median": med, "call_us_min": min(us), "call_us_max": max(us),
                    "back_to_back_us": _timed(fn, a.reps) * 1e3, "GB_s": nbytes / (med * 1e-6) / 1e9, "launches": launch_us(fn, 5),
                    "edt_call_us_median": emed, "edt_GB_s": B * H * W * 5.0 / (emed * 1e-6) / 1e9, "edt_launches": launch_us(edt, 5),
                    "host_copy_us_median": statistics.median(h[0] for h in host), "host_scipy_us_median": statistics.median(h[1] for h in host),
                    "host_pairs": host[0][2], "host_over_device": hmed / med}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
