"""Measurements of the defect skeletons (csrc/skeleton.hip, uaps_amd/skeleton.py), DESIGN.md section 3.27.

Shapes 16 x 256 x 256 and 2 x 1024 x 1024 at C = 4 (classes 1..3 thinned), on four fillings
  sparse   about 10 blobs per image, the realistic case
  cracks   class noise at density 0.03 dilated by a 3 x 3 square: thin, branched, touching webs
  rings    about 8 rings per image, two to five pixels wide
  one      one component filling every image (64 iterations do not reach its fixed point)
Per case:
  skeletonize at max_iters = 64: events around each call (median of --reps calls), the first thinning launch alone (events on its
    dispatch), and the call at max_iters = 128 -- every launch it adds finds its image converged (except on `one`), so the
    difference over the added launches is what a converged launch costs
  skeleton_descriptors with and without a plane (call and kernel; the plane is formed outside the timed region)
  s_sweep_call_us     the call at S = 2, 4, 8, 16, 32 sub-iterations a launch, at the band height the library chooses for that S
  band_sweep_call_us  the call at the chosen S and forced band heights of 8, 16, 32, 64 rows
  torch     the same rule composed from torch ops on the device: shifted slices and boolean ops per sub-iteration on the one-hot
            planes, with a host check for convergence every iteration (at most 64 iterations)
  host      the copy to the host plus the package's numpy path on 16 threads (once)
Nothing gates on these times.

    python tools/bench_skeleton.py [--reps 50] [--out profiles/skeleton_bench.json]

Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _timing import _kernel_ms  # noqa: E402

C = 4
SHAPES = ((16, 256, 256), (2, 1024, 1024))
S_SWEEP, BAND_SWEEP = (2, 4, 8, 16, 32), (8, 16, 32, 64)


def fillings(B, H, W):
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    sparse, rings = np.zeros((B, H, W), dtype=np.int64), np.zeros((B, H, W), dtype=np.int64)
    for b in range(B):
        for _ in range(10):
            cy, cx, ry, rx = rng.integers(0, H), rng.integers(0, W), rng.integers(3, H // 10), rng.integers(3, W // 10)
            sparse[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = rng.integers(1, C)
        for _ in range(8):
            cy, cx, r, w = rng.integers(0, H), rng.integers(0, W), rng.integers(6, H // 6), rng.integers(2, 6)
            d = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
            rings[b][(d <= r) & (d >= r - w)] = rng.integers(1, C)
    salt = rng.random((B, H, W)) < 0.03
    pad = np.pad(salt, ((0, 0), (1, 1), (1, 1)))
    grown = np.zeros_like(salt)
    for dy in range(3):
        for dx in range(3):
            grown |= pad[:, dy:dy + H, dx:dx + W]
    cracks = np.where(grown, np.kron(rng.integers(1, C, (B, H // 64, W // 64)), np.ones((64, 64), dtype=np.int64)), 0).astype(np.int64)
    return {"sparse": sparse, "cracks": cracks, "rings": rings, "one": np.ones((B, H, W), dtype=np.int64)}


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


def med_us(fn, reps):
    return statistics.median(call_us(fn, reps))


def _shift(p, dy, dx):
    """p[..., y + dy, x + dx], False outside."""
    out = torch.zeros_like(p)
    H, W = p.shape[-2:]
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[..., yd, xd] = p[..., ys, xs]
    return out


def torch_composition(mask, max_iters=64):
    """Guo-Hall on the one-hot planes of classes 1..C-1 from torch ops; the host decides after every iteration whether to go on."""
    p = torch.nn.functional.one_hot(mask, C)[..., 1:].permute(0, 3, 1, 2).bool()
    for _ in range(max_iters):
        before = p
        for second in (False, True):
            P2, P3, P4, P5 = _shift(p, -1, 0), _shift(p, -1, 1), _shift(p, 0, 1), _shift(p, 1, 1)
            P6, P7, P8, P9 = _shift(p, 1, 0), _shift(p, 1, -1), _shift(p, 0, -1), _shift(p, -1, -1)
            i8 = lambda t: t.to(torch.int8)
            Cn = i8(~P2 & (P3 | P4)) + i8(~P4 & (P5 | P6)) + i8(~P6 & (P7 | P8)) + i8(~P8 & (P9 | P2))
            N = torch.minimum(i8(P9 | P2) + i8(P3 | P4) + i8(P5 | P6) + i8(P7 | P8), i8(P2 | P3) + i8(P4 | P5) + i8(P6 | P7) + i8(P8 | P9))
            third = ((P6 | P7 | ~P9) & P8) if second else ((P2 | P3 | ~P5) & P4)
            p = p & ~((Cn == 1) & (N >= 2) & (N <= 3) & ~third)
        if not bool((before != p).any().item()):
            break
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uaps_amd import distance_transform_sq, label_instances, skeleton_descriptors, skeletonize
    from uaps_amd.skeleton import band_rows
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    res = {"classes": C, "reps": a.reps, "device": torch.cuda.get_device_name(0), "max_iters": 64, "host_threads": 16, "cases": []}
    for B, H, W in SHAPES:
        for fname, m in fillings(B, H, W).items():
            mask = torch.from_numpy(m).to(dev)
            thin = lambda **kw: skeletonize(mask, C, **kw)
            skel = thin()
            planes = torch_composition(mask)
            for c in range(1, C):                       # the composition computes the same skeleton
                assert torch.equal(planes[:, c - 1], skel.mask == c), (fname, c)
            us = call_us(thin, a.reps)
            us128 = med_us(lambda: thin(max_iters=128), a.reps)
            chosen_s = 8
            launches64, launches128 = 2 * 64 // chosen_s, 2 * 128 // chosen_s
            inst = label_instances(mask, max_instances=256)
            plane = distance_transform_sq(inst.labels)
            with_plane = lambda: skeleton_descriptors(inst, skel, _plane=plane)
            bare = lambda: skeleton_descriptors(inst, skel, thickness=False)
            t0 = time.perf_counter()
            host_mask = mask.cpu()
            t1 = time.perf_counter()
            host = skeletonize(host_mask, C)
            t2 = time.perf_counter()
            assert torch.equal(host.mask, skel.mask.cpu())
            torch_us = call_us(lambda: torch_composition(mask), 3)
            res["cases"].append({
                "shape": [B, H, W], "filling": fname, "converged": skel.converged.tolist(),
                "removed_pixels": int((skel.mask != mask).sum()), "skeleton_pixels": int((skel.mask > 0).sum()),
                "band_rows": band_rows(H, W, C - 1), "sub_iters": chosen_s, "thin_launches": launches64,
                "skeletonize_call_us_median": statistics.median(us), "skeletonize_call_us_min": min(us),
                "first_thin_launch_kernel_us_mean": _kernel_ms(thin, a.reps) * 1e3,
                "skeletonize_128_call_us_median": us128,
                "added_launch_us": (us128 - statistics.median(us)) / (launches128 - launches64),
                "descriptors_plane_call_us_median": med_us(with_plane, a.reps), "descriptors_plane_kernel_us_mean": _kernel_ms(with_plane, a.reps) * 1e3,
                "descriptors_bare_call_us_median": med_us(bare, a.reps), "descriptors_bare_kernel_us_mean": _kernel_ms(bare, a.reps) * 1e3,
                "descriptors_thickness_call_us_median": med_us(lambda: skeleton_descriptors(inst, skel), a.reps),
                "s_sweep_call_us": {str(s): med_us(lambda: thin(_sub_iters=s), a.reps) for s in S_SWEEP},
                "s_sweep_band_rows": {str(s): band_rows(H, W, C - 1, s) for s in S_SWEEP},
                "band_sweep_call_us": {str(r): med_us(lambda: thin(_band_rows=r), a.reps) for r in BAND_SWEEP},
                "torch_composition_us_median": statistics.median(torch_us),
                "host_copy_us": (t1 - t0) * 1e6, "host_numpy_us": (t2 - t1) * 1e6})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
