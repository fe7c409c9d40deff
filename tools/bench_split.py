"""Measurements of the splitting of touching defects (csrc/split.hip, uaps_amd/split.py), DESIGN.md section 3.34.

Shapes 16 x 256 x 256 and 2 x 1024 x 1024, 8-connectivity, four fillings:
  pairs    about ten pairs of overlapping discs per 256 x 256 pixels (radii 8..20), distance form at radius 5: the realistic case
  noise    class noise at density 0.5, distance form at radius 1 (every defect pixel is a marker pixel): the most markers, no round
  full     one component filling every image with ONE marker pixel in its corner (marker form): the longest straight front
  spiral   a one-pixel-wide rectangular spiral (pitch H / 16) with a marker at each end (marker form): the most working rounds
max_iters is the number of rounds the filling needs (found by the composition below) plus one, at least 256 (the default).
Each case is timed as
  call         events around each of `reps` calls, median and minimum, at the default S and tile
  sweep        the same median (10 calls) at S in {2, 8, 16} x tiles (32, 32), (16, 64), (64, 16), (8, 128); null where the tile does
               not fit the LDS budget
  launches     the median microseconds of every kernel of the call (torch.profiler's kernel records) and their share of the sum
  composition  the same rounds composed on the device from torch ops (shifted views of a padded plane, eq / where / minimum) between
               two label_instances calls; its labels and counts are asserted equal to the call's.  Timed without its stop test.
  host         the device-to-host copy, then the reference of tests/split_ref.py image by image on 16 threads (null where the flood
               would take minutes: more than 2e9 pixels x (rounds or defects an image))
Nothing gates on these times.  No hardware counters were collected: what bounds the call is read off the launch table (the share of
the growth launches, their count and their mean duration against an empty launch's) and is stated as inferred.

    python tools/bench_split.py [--reps 50] [--out profiles/split_bench.json]

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

from bench_instances import call_us, launch_us  # noqa: E402

SHAPES = ((16, 256, 256), (2, 1024, 1024))
SWEEP_S = (2, 8, 16)
SWEEP_TILES = ((32, 32), (16, 64), (64, 16), (8, 128))
C = 4


def spiral(H, W, pitch):
    """A one-pixel-wide rectangular spiral whose windings lie `pitch` apart, from the outside in; its two end pixels."""
    m = np.zeros((H, W), dtype=np.int64)
    top, bottom, left, right = 0, H - 1, 0, W - 1
    y, x, d = 0, 0, 0
    path = [(0, 0)]
    while True:
        n = (right - x, bottom - y, x - left, y - top)[d]       # steps to the bound this leg runs to
        if n <= 0:
            break
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        for _ in range(n):
            y, x = y + dy, x + dx
            path.append((y, x))
        if d == 0:
            top += pitch
        elif d == 1:
            right -= pitch
        elif d == 2:
            bottom -= pitch
        else:
            left += pitch
        d = (d + 1) % 4
    for py, px in path:
        m[py, px] = 1
    ends = np.zeros((H, W), dtype=bool)
    ends[path[0]] = ends[path[-1]] = True
    return m, ends


def fillings(B, H, W):
    """name -> (mask int64 [B,H,W], markers bool [B,H,W] or None, radius or None)."""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    pairs = np.zeros((B, H, W), dtype=np.int64)
    for b in range(B):
        for _ in range(10 * (H * W) // (256 * 256)):
            r = int(rng.integers(8, 21))
            cy, cx, d, th = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(r, 2 * r - 2), rng.uniform(0, 2 * np.pi)
            c = int(rng.integers(1, C))
            for py, px in ((cy, cx), (cy + d * np.sin(th), cx + d * np.cos(th))):
                pairs[b][(yy - py) ** 2 + (xx - px) ** 2 <= r * r] = c
    noise = np.where(rng.random((B, H, W)) < 0.5, rng.integers(1, C, (B, H, W)), 0).astype(np.int64)
    corner = np.zeros((B, H, W), dtype=bool)
    corner[:, 0, 0] = True
    sp, ends = spiral(H, W, H // 16)
    return {"pairs": (pairs, None, 5.0), "noise": (noise, None, 1.0), "full": (np.ones((B, H, W), dtype=np.int64), corner, None),
            "spiral": (np.repeat(sp[None], B, 0), np.repeat(ends[None], B, 0), None)}


def _shifted(p, dy, dx, H, W):
    return p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def composed(inst, marker, rounds=None):
    """The same pieces from what the package had before this entry point, all on the device: (labels, count, rounds).  rounds=None:
    until nothing changes (one host read a round); else exactly that many rounds and no host read."""
    from uaps_amd import label_instances
    lab = inst.labels.long()
    B, H, W = lab.shape
    own = label_instances(torch.where((lab > 0) & marker, lab, torch.zeros_like(lab)), max_instances=1).labels.long()
    none = torch.full_like(own, 2 ** 40)
    pl = torch.nn.functional.pad(lab, (1, 1, 1, 1))
    done = 0
    while rounds is None or done < rounds:
        po = torch.nn.functional.pad(own, (1, 1, 1, 1))
        best = none
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    nl, no = _shifted(pl, dy, dx, H, W), _shifted(po, dy, dx, H, W)
                    best = torch.minimum(best, torch.where((nl == lab) & (no > 0), no, none))
        take = (lab > 0) & (own == 0) & (best < none)
        if rounds is None and not bool(take.any()):
            break
        own = torch.where(take, best, own)
        done += 1
    res = label_instances(torch.where(lab > 0, (lab << 32) | own, torch.zeros_like(lab)), max_instances=1)
    return res.labels, res.count, done


def host_today(inst, marker, max_iters, pool):
    """What the package's user does without this feature: copy, then the flood of tests/split_ref.py per image."""
    import split_ref
    t0 = time.perf_counter()
    labels, table, mk = inst.labels.cpu().numpy(), inst.table.cpu().numpy(), marker.cpu().numpy()
    t1 = time.perf_counter()
    list(pool.map(lambda b: split_ref.split_batch(labels[b:b + 1], table[b:b + 1], mk[b:b + 1], max_iters=max_iters), range(labels.shape[0])))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6


def write(res, out):
    line = json.dumps(res)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))         # the scipy reference of the tests
    from uaps_amd import _lib, label_instances, split_instances
    from uaps_amd.split import band_rows
    from uaps_amd.surface import distance_transform_sq
    dev = torch.device("cuda:0")
    res = {"connectivity": 8, "reps": a.reps, "device": torch.cuda.get_device_name(0), "host_threads": 16, "counters_collected": False,
           "default_tile": list(band_rows(256, 256)), "bound": "launch count x rounds, inferred from the launch table", "cases": []}
    with ThreadPoolExecutor(16) as pool:
        for B, H, W in SHAPES:
            for name, (mask, markers, radius) in fillings(B, H, W).items():
                inst = label_instances(torch.from_numpy(mask).to(dev), max_instances=4096)
                if markers is None:
                    marker = distance_transform_sq(inst.labels) >= int(np.ceil(radius * radius))
                    how = {"radius": radius}
                else:
                    marker = torch.from_numpy(markers).to(dev)
                    how = {"markers": marker}
                labels_c, count_c, rounds = composed(inst, marker)
                iters = max(256, rounds + 1)
                fn = lambda **kw: split_instances(inst, max_iters=iters, **how, **kw)
                out = fn()
                assert bool(out.converged.all()) and torch.equal(out.instances.labels, labels_c) and torch.equal(out.instances.count, count_c)
                us = call_us(fn, a.reps)
                sweep = {}
                for S in SWEEP_S:
                    for tile in SWEEP_TILES:
                        key = f"S{S}_tile{tile[0]}x{tile[1]}"
                        try:
                            f2 = lambda: fn(_sub_iters=S, _band_rows=tile)
                            assert torch.equal(f2().instances.labels, out.instances.labels)
                            sweep[key] = statistics.median(call_us(f2, 10))
                        except _lib.UapsHipError:
                            sweep[key] = None
                launches = launch_us(fn, 5)
                if launches and "error" not in launches:
                    total = sum(v["median_us"] * v["launches_per_call"] for v in launches.values())
                    for v in launches.values():
                        v["share"] = v["median_us"] * v["launches_per_call"] / total
                comp = statistics.median(call_us(lambda: composed(inst, marker, rounds), 3))
                # the flood costs a frame a round and marker, and a frame a defect
                heavy = float(max(rounds, int(inst.count.max()))) * H * W > 2e9
                host = None if heavy else host_today(inst, marker, iters, pool)
                res["cases"].append({
                    "shape": [B, H, W], "filling": name, "form": "distance" if markers is None else "markers", "radius": radius,
                    "defects": int(inst.count.sum()), "pieces": int(out.instances.count.sum()), "rounds": rounds, "max_iters": iters,
                    "growth_launches": -(-iters // 8), "call_us_median": statistics.median(us), "call_us_min": min(us),
                    "sweep_us_median": sweep, "launches": launches, "composition_us_median": comp,
                    "host_copy_us": None if host is None else host[0], "host_reference_us": None if host is None else host[1]})
                print(f"{B}x{H}x{W} {name}: {res['cases'][-1]['call_us_median']:.0f} us, {rounds} rounds", file=sys.stderr, flush=True)
                write(res, a.out)                            # (what is measured so far survives an interrupted run)
    print(write(res, a.out))


if __name__ == "__main__":
    main()
