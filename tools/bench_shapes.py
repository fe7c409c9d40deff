"""Measurements of the shape descriptors (csrc/shapes.hip, uaps_amd/shapes.py), DESIGN.md section 3.26.

Shapes 16 x 256 x 256 and 2 x 1024 x 1024 at C = 4, 8-connectivity, on the labels of label_instances over the four fillings of the
component bench
  sparse   about 10 blobs per image, the realistic case
  noise    class noise at density 0.5: far more components than rows, most labels above M
  one      one component filling every image: every run of an image goes to one table row
  rings    about 10 annuli per image with salt and pepper
with and without a plane (the squared distance transform of the labels), in BOTH flush forms on the same labels:
  lds      M = 256: a workgroup adds its runs into a copy of the image's table in LDS and sends the non-zero words
  direct   M = 257: the runs' first lanes send global atomics (one more table row; the first 256 rows are asserted equal)
Each is timed as
  call         events around each of `reps` calls, median and minimum
  launches     the median microseconds of every kernel of the call (torch.profiler's kernel records; null where it reports none)
and the same arithmetic two other ways, at M = 256:
  torch        composed from torch ops on the device: index_add_ over the labels for the sums, shifted comparisons of the padded
               labels for the quads, scatter_reduce for the plane's maximum (asserted equal to the kernel's table)
  host         the device-to-host copy, then numpy per image on 16 threads (the package's CPU path) and scipy.ndimage.sum_labels for
               the five moment sums alone
Nothing gates on these times.  "bytes" is 4 bytes a pixel (8 with a plane) plus the table written once; the rate is formed on the
accumulate kernel's time where the profiler reports it, on the call otherwise.

    python tools/bench_shapes.py [--reps 50] [--out profiles/shapes_bench.json]

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
from bench_instances import call_us, launch_us  # noqa: E402

C = 4
M = 256
SHAPES = ((16, 256, 256), (2, 1024, 1024))


def torch_composed(labels, plane, rows):
    """The table from torch ops alone; labels int32 [B,H,W] on the device."""
    B, H, W = labels.shape
    dev = labels.device
    lab = labels.long()
    lab = torch.where((lab >= 1) & (lab <= rows), lab, torch.zeros_like(lab))
    base = (torch.arange(B, device=dev) * (rows + 1)).view(B, 1, 1)
    out = torch.zeros((B * (rows + 1), 11), dtype=torch.int64, device=dev)          # row 0 of every image takes what has no row
    y = torch.arange(H, device=dev).view(1, H, 1).expand(B, H, W)
    x = torch.arange(W, device=dev).view(1, 1, W).expand(B, H, W)
    vals = torch.stack([y, x, y * y, x * y, x * x], dim=-1).reshape(-1, 5)
    key = (lab + base).reshape(-1)
    out[:, 0:5] = torch.zeros_like(out[:, 0:5]).index_add_(0, key, vals)
    if plane is not None:
        p = plane.long().clamp(min=0).reshape(-1)
        out[:, 10] = torch.zeros_like(out[:, 10]).index_add_(0, key, p)
        out[:, 9] = torch.zeros_like(out[:, 9]).scatter_reduce(0, key, p, "amax")
    pad = torch.nn.functional.pad(lab, (1, 1, 1, 1))
    c = [pad[:, :-1, :-1], pad[:, :-1, 1:], pad[:, 1:, :-1], pad[:, 1:, 1:]]
    diag = (3, 2, 1, 0)
    for i in range(4):
        first = c[i] > 0
        for j in range(i):
            first = first & (c[j] != c[i])
        same = [c[j] == c[i] for j in range(4)]
        n = same[0].long() + same[1] + same[2] + same[3]
        d = same[diag[i]]
        hot = torch.stack([n == 1, (n == 2) & ~d, n == 3, (n == 2) & d], dim=-1) & first.unsqueeze(-1)
        out[:, 5:9] += torch.zeros_like(out[:, 5:9]).index_add_(0, (c[i] + base).reshape(-1), hot.reshape(-1, 4).long())
    return out.view(B, rows + 1, 11)[:, 1:].contiguous()


def host_today(labels_dev, plane_dev, pool):
    """What the package's user does without this feature: copy, then numpy per image; and scipy for the five sums."""
    from scipy import ndimage
    from uaps_amd.shapes import _shapes_cpu
    t0 = time.perf_counter()
    labels = labels_dev.cpu().numpy()
    plane = None if plane_dev is None else plane_dev.cpu().numpy()
    t1 = time.perf_counter()
    list(pool.map(lambda b: _shapes_cpu(labels[b:b + 1], None if plane is None else plane[b:b + 1], M), range(labels.shape[0])))
    t2 = time.perf_counter()
    H, W = labels.shape[1:]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    idx = np.arange(1, M + 1)

    def sums(b):
        lab = np.where(labels[b] <= M, labels[b], 0)
        return [ndimage.sum_labels(v, lab, idx) for v in (yy, xx, yy * yy, xx * yy, xx * xx)]
    list(pool.map(sums, range(labels.shape[0])))
    t3 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6, (t3 - t2) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uaps_amd import distance_transform_sq, label_instances, shape_descriptors
    dev = torch.device("cuda:0")
    res = {"classes": C, "connectivity": 8, "max_instances": M, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "host_threads": 16, "cases": []}
    with ThreadPoolExecutor(16) as pool:
        for B, H, W in SHAPES:
            for fname, m in fillings(B, H, W).items():
                mask = torch.from_numpy(m).to(dev)
                inst = {rows: label_instances(mask, max_instances=rows) for rows in (M, M + 1)}
                assert torch.equal(inst[M].labels, inst[M + 1].labels)
                dist = distance_transform_sq(inst[M].labels)
                for with_plane in (False, True):
                    plane = dist if with_plane else None
                    nbytes = float(B * H * W) * (8.0 if with_plane else 4.0) + 88.0 * B * M
                    case = {"shape": [B, H, W], "filling": fname, "plane": with_plane, "components_max": int(inst[M].count.max()),
                            "bytes": nbytes}
                    tables = {}
                    for form, rows in (("lds", M), ("direct", M + 1)):
                        fn = lambda: shape_descriptors(inst[rows], plane)
                        tables[form] = fn().table
                        us = call_us(fn, a.reps)
                        launches = launch_us(fn, 10)
                        acc = None
                        if launches and "error" not in launches:
                            acc = next((v["median_us"] for k, v in launches.items() if k.startswith("shape_accumulate")), None)
                        case[form] = {"call_us_median": statistics.median(us), "call_us_min": min(us), "launches": launches,
                                      "accumulate_us_median": acc,
                                      "GB_s": nbytes / ((acc or statistics.median(us)) * 1e-6) / 1e9, "rate_on": "kernel" if acc else "call"}
                    assert torch.equal(tables["direct"][:, :M], tables["lds"]), (B, H, W, fname, with_plane)
                    composed = lambda: torch_composed(inst[M].labels, plane, M)
                    assert torch.equal(composed(), tables["lds"])
                    case["torch_ops_us_median"] = statistics.median(call_us(composed, max(5, a.reps // 5)))
                    host = [host_today(inst[M].labels, plane, pool) for _ in range(3)]
                    case["host_copy_us_median"] = statistics.median(h[0] for h in host)
                    case["host_numpy_us_median"] = statistics.median(h[1] for h in host)
                    case["host_scipy_sums_us_median"] = statistics.median(h[2] for h in host)
                    res["cases"].append(case)
                    print(B, H, W, fname, with_plane, case["lds"]["call_us_median"], case["direct"]["call_us_median"], file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
