"""Measurements of defect detection matching (csrc/detect.hip, uaps_amd/detection.py) at 16 x 256 x 256 and 2 x 1024 x 1024, C = 4,
8-connectivity, 256 table rows on both sides, T = 10 (COCO's 0.50 .. 0.95), on the three fillings of tools/bench_match.py (DESIGN.md
section 3.31):
  sparse   about 10 blobs per image against the same blobs moved by (2, 3): the realistic case
  noise    class noise against itself with 10 % of the pixels drawn again: both tables overflow, so every one of the 256 rows holds a
           detection -- the longest sequential sweep the table size allows
  one      one component filling every image, on both sides

Per shape and filling: the median microseconds of one detection_match call alone (events around each call; the two label_instances
calls are made once, outside) and of each of its launches (torch.profiler's kernel records; null where the profiler reports none) --
sweep_kernel's is the sequential part --, and on the same inputs in the same session what the package offered before: ten
match_instances calls, one per threshold (the cheapest way to ten thresholds at or above 0.5; they pay the pair count ten times), and
the copy to the host plus the module's numpy path, the images spread over 16 threads.

    python tools/bench_detect.py [--reps 50] [--out profiles/detect_bench.json]

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

import torch  # noqa: E402

import bench_instances  # noqa: E402
from _timing import _timed  # noqa: E402
from bench_instances import C, M, call_us, launch_us  # noqa: E402
from bench_match import predictions  # noqa: E402

SHAPES = ((16, 256, 256), (2, 1024, 1024))
TABLES = ("rank", "pred_match", "pred_inter", "target_match", "counts")


def fillings_at(B, H, W):
    """bench_instances.fillings() and bench_match.predictions() at another shape (both read the module's B, H, W when called)."""
    saved = bench_instances.B, bench_instances.H, bench_instances.W
    bench_instances.B, bench_instances.H, bench_instances.W = B, H, W
    try:
        fill = bench_instances.fillings()
        return fill, predictions(fill)
    finally:
        bench_instances.B, bench_instances.H, bench_instances.W = saved


def host_today(ip, ig, pool, thresholds):
    """The copy to the host, then the module's numpy path image by image on the pool's threads."""
    from uaps_amd import InstanceResult, detection_match
    t0 = time.perf_counter()
    hp, hg = [t.cpu() for t in ip[:3]], [t.cpu() for t in ig[:3]]
    t1 = time.perf_counter()
    one = lambda b: detection_match(InstanceResult(*[t[b:b + 1] for t in hp], 1), InstanceResult(*[t[b:b + 1] for t in hg]), C,
                                    iou_thresholds=thresholds)
    res = list(pool.map(one, range(hp[0].shape[0])))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uaps_amd import COCO_THRESHOLDS, detection_match, label_instances, match_instances
    dev = torch.device("cuda:0")
    res = {"classes": C, "max_instances": M, "connectivity": 8, "thresholds": list(COCO_THRESHOLDS), "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "host_threads": 16, "shapes": {}}
    with ThreadPoolExecutor(16) as pool:
        for B, H, W in SHAPES:
            fill, preds = fillings_at(B, H, W)
            torch.manual_seed(0)
            conf = torch.rand(B, H, W, device=dev)
            per = res["shapes"][f"{B}x{H}x{W}"] = {"pair_matrix_bytes": B * M * M * 4, "fillings": {}}
            for name, gt in fill.items():
                ip = label_instances(torch.from_numpy(preds[name]).to(dev), maps=(conf,), connectivity=8, max_instances=M)
                ig = label_instances(torch.from_numpy(gt).to(dev), connectivity=8, max_instances=M)
                fn = lambda: detection_match(ip, ig, C)
                ten = lambda: [match_instances(ip, ig, C, iou_threshold=t) for t in COCO_THRESHOLDS]
                r = fn()
                # the two agree wherever no pair sits exactly on a threshold (match_instances is strict): reported, not required
                tp_ten = torch.stack([m.counts[..., 0] for m in ten()], dim=-1)
                us, us_ten = call_us(fn, a.reps), call_us(ten, a.reps)
                host = [host_today(ip, ig, pool, COCO_THRESHOLDS) for _ in range(3)]
                same_host = all(torch.equal(getattr(r, n).cpu(), torch.cat([getattr(h, n) for h in host[0][2]])) for n in TABLES)
                launches = launch_us(fn, 10)
                per["fillings"][name] = {
                    "components_per_image_pred": float(ip.count.float().mean()), "components_per_image_gt": float(ig.count.float().mean()),
                    "detections_in_sequence": int((r.rank >= 0).sum()), "images_valid": int(r.valid.sum()),
                    "tp_at_0.50": int(r.counts[..., 0].sum()), "tp_at_0.95": int(r.counts[..., 9].sum()),
                    "call_us_median": statistics.median(us), "call_us_min": min(us), "call_us_max": max(us),
                    "back_to_back_us": _timed(fn, a.reps) * 1e3, "launches": launches,
                    "sweep_us_median": (launches or {}).get("sweep_kernel"),
                    "ten_match_instances_us_median": statistics.median(us_ten), "ten_match_instances_us_min": min(us_ten),
                    "ten_match_instances_tp_equal": bool(torch.equal(tp_ten, r.counts[..., :10])),
                    "host_copy_us_median": statistics.median(h[0] for h in host),
                    "host_numpy_us_median": statistics.median(h[1] for h in host), "host_equal": same_host}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
