"""Measurements of the mask clean-up morphology (csrc/morph.hip, uaps_amd/morphology.py), DESIGN.md section 3.24.

Shapes 16 x 256 x 256 and 2 x 1024 x 1024 at C = 4; chains
  open1        [("open", "disk", 1)]
  open2close2  [("open", "disk", 2), ("close", "square", 2)]
  open8        [("open", "disk", 8)]
on three fillings
  sparse   about 10 blobs per image, the realistic case
  noise    class noise at density 0.5
  one      one component filling every image
Each case is timed four ways:
  fused      the chain in one launch (events around each call; the kernel alone, events on its dispatch)
  per_step   the same chain as one uaps_morphology call per step
  torch      a composition of max_pool2d on one-hot planes -- BINARY semantics only: every class plane on its own with the same border
             rule, square footprints in place of disks, and no rule for two classes that grow into one pixel; it is what a user can
             write today, not the same result
  host       the device-to-host copy, then scipy.ndimage per image and class on 16 threads (binary planes, no combine either)
On the sparse filling the kernel is also timed at forced band heights of 4, 8, 16 and 32 rows ("band_sweep_kernel_us"): the
measurement behind the library's band-height rule.
Nothing gates on these times.  GB/s is the rate on the algorithmic 16 bytes per pixel (the int64 map read once and written once).

    python tools/bench_morph.py [--reps 50] [--out profiles/morph_bench.json]

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

C = 4
SHAPES = ((16, 256, 256), (2, 1024, 1024))
CHAINS = {"open1": [("open", "disk", 1)], "open2close2": [("open", "disk", 2), ("close", "square", 2)], "open8": [("open", "disk", 8)]}


def fillings(B, H, W):
    rng = np.random.default_rng(0)
    sparse = np.zeros((B, H, W), dtype=np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        for _ in range(10):
            cy, cx, ry, rx = rng.integers(0, H), rng.integers(0, W), rng.integers(3, H // 10), rng.integers(3, W // 10)
            sparse[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = rng.integers(1, C)
    noise = np.where(rng.random((B, H, W)) < 0.5, rng.integers(1, C, (B, H, W)), 0).astype(np.int64)
    return {"sparse": sparse, "noise": noise, "one": np.ones((B, H, W), dtype=np.int64)}


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


def torch_composition(mask, steps):
    """Binary planes through max_pool2d: dilation = max over the square window (padding counts as background), erosion = 1 - the
    dilation of the complement (padding counts as foreground)."""
    planes = torch.nn.functional.one_hot(mask, C)[..., 1:].permute(0, 3, 1, 2).float()
    dil = lambda p, r: torch.nn.functional.max_pool2d(p, 2 * r + 1, 1, r)
    ero = lambda p, r: 1.0 - dil(1.0 - p, r)
    for op, _, r in steps:
        if op == "open":
            planes = dil(ero(planes, r), r)
        elif op == "close":
            planes = ero(dil(planes, r), r)
        elif op == "erode":
            planes = ero(planes, r)
        elif op == "dilate":
            planes = dil(planes, r)
        else:
            planes = planes * (1.0 - ero(planes, r))
    return planes


def host_today(mask_dev, steps, pool):
    import morph_ref
    t0 = time.perf_counter()
    mask = mask_dev.cpu().numpy()
    t1 = time.perf_counter()
    S = [(op, morph_ref.footprint(fp, r)) for op, fp, r in steps]

    def image(b):
        for c in range(1, C):
            p = mask[b] == c
            for op, s in S:
                p = morph_ref.step_plane(p, op, s)
        return 0
    list(pool.map(image, range(mask.shape[0])))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))         # the scipy footprints of the tests' reference
    from uaps_amd import morphology
    from uaps_amd.morphology import band_rows, chain_reach
    dev = torch.device("cuda:0")
    res = {"classes": C, "reps": a.reps, "device": torch.cuda.get_device_name(0), "bytes_per_pixel": 16, "host_threads": 16, "cases": []}
    with ThreadPoolExecutor(16) as pool:
        for B, H, W in SHAPES:
            nbytes = 16.0 * B * H * W
            for fname, m in fillings(B, H, W).items():
                mask = torch.from_numpy(m).to(dev)
                for cname, steps in CHAINS.items():
                    fused = lambda: morphology(mask, steps, C)

                    def per_step():
                        out = mask
                        for s in steps:
                            out = morphology(out, [s], C)
                        return out
                    assert torch.equal(fused(), per_step())
                    us = call_us(fused, a.reps)
                    med = statistics.median(us)
                    kern = _kernel_ms(fused, a.reps) * 1e3
                    host = [host_today(mask, steps, pool) for _ in range(3)]
                    sweep = None
                    if fname == "sparse":
                        sweep = {str(rows): _kernel_ms(lambda: morphology(mask, steps, C, _band_rows=rows), a.reps) * 1e3 for rows in (4, 8, 16, 32)}
                    res["cases"].append({
                        "shape": [B, H, W], "filling": fname, "chain": cname, "reach": chain_reach(steps),
                        "band_rows": band_rows(H, W, C - 1, chain_reach(steps)),
                        "changed_pixels": int((fused() != mask).sum()),
                        "fused_call_us_median": med, "fused_call_us_min": min(us), "fused_kernel_us_mean": kern,
                        "fused_back_to_back_us": _timed(fused, a.reps) * 1e3,
                        "band_sweep_kernel_us": sweep,
                        "GB_s_call": nbytes / (med * 1e-6) / 1e9, "GB_s_kernel": nbytes / (kern * 1e-6) / 1e9,
                        "per_step_call_us_median": statistics.median(call_us(per_step, a.reps)),
                        "torch_maxpool_binary_us_median": statistics.median(call_us(lambda: torch_composition(mask, steps), a.reps)),
                        "host_copy_us_median": statistics.median(h[0] for h in host),
                        "host_scipy_us_median": statistics.median(h[1] for h in host)})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
