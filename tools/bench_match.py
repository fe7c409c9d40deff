"""Measurements of defect matching against ground truth (csrc/match.hip, uaps_amd/matching.py) at the workload's shape, 16 x 256 x 256,
C = 4, 8-connectivity, max_instances = 256 on both sides, on the three fillings of tools/bench_instances.py:
  sparse   about 10 blobs per image against the same blobs moved by (2, 3): the realistic case
  noise    class noise at density 0.5 against itself with 10 % of the pixels drawn again: both tables overflow (about 14,000 components
           per image, 256 rows), so this is the time of the overflow path
  one      one component filling every image, on both sides: every add of an image lands on one word of the pair matrix

Per filling: the median microseconds of one match_instances call alone (events around each call; the two label_instances calls are
made once, outside), the median microseconds of each of its launches (torch.profiler's kernel records; null where the profiler reports
none), the same arithmetic composed from torch ops on the device (torch.bincount over the flattened keys with minlength = B * Mp * Mg,
then amax / argmax / sum and the comparisons), and the copy to the host plus the module's numpy path, the images spread over 16
threads.  Beside them the time of zeroing the WHOLE pair matrix (what zero_kernel's corner rule is an alternative to).

    python tools/bench_match.py [--reps 50] [--out profiles/match_bench.json]

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
from bench_instances import B, C, H, M, W, call_us, fillings, launch_us  # noqa: E402

THR = 0.5


def predictions(fill):
    """The prediction that goes with every ground-truth filling."""
    rng = np.random.default_rng(1)
    noise = fill["noise"]
    return {"sparse": np.roll(fill["sparse"], (2, 3), axis=(1, 2)), "one": fill["one"].copy(),
            "noise": np.where(rng.random(noise.shape) < 0.1, rng.integers(0, C, noise.shape), noise).astype(np.int64)}


def torch_composition(ip, ig):
    """The tables of match_instances from torch ops: what a user composes on the device without the kernels."""
    Mp, Mg = ip.max_instances, ig.max_instances
    p, g = ip.labels.reshape(B, -1).long(), ig.labels.reshape(B, -1).long()
    ok = (p >= 1) & (p <= Mp) & (g >= 1) & (g <= Mg)
    pi, gi = (p - 1).clamp(0, Mp - 1), (g - 1).clamp(0, Mg - 1)
    ok &= torch.gather(ip.table[..., 0], 1, pi) == torch.gather(ig.table[..., 0], 1, gi)
    key = (torch.arange(B, device=p.device)[:, None] * Mp + pi) * Mg + gi
    inter = torch.bincount(torch.where(ok, key, torch.full_like(key, B * Mp * Mg)).reshape(-1), minlength=B * Mp * Mg + 1)[:-1].view(B, Mp, Mg)
    rows_p = torch.arange(Mp, device=p.device)[None] < ip.count.clamp(max=Mp)[:, None]
    rows_g = torch.arange(Mg, device=p.device)[None] < ig.count.clamp(max=Mg)[:, None]
    out = []
    for dim, mine, other, rows in ((2, ip, ig, rows_p), (1, ig, ip, rows_g)):
        top, best = inter.max(dim=dim)                          # (the first maximum: the lowest number on ties)
        union = mine.table[..., 1] + torch.gather(other.table[..., 1], 1, best) - top
        matched = (top > 0) & (top.double() > THR * union.double())
        t = torch.stack([torch.where(top > 0, best + 1, torch.zeros_like(best)), top, inter.sum(dim=dim), matched.long()], dim=2)
        out.append(torch.where(rows[..., None], t, torch.zeros_like(t)))
    cls = torch.arange(C, device=p.device)[None, :, None]
    of_p, of_g = (ip.table[..., 0][:, None] == cls) & rows_p[:, None], (ig.table[..., 0][:, None] == cls) & rows_g[:, None]
    counts = torch.stack([(of_g & (out[1][..., 3] > 0)[:, None]).sum(2), of_p.sum(2), of_g.sum(2)], dim=2)
    return out[0], out[1], counts


def host_today(ip, ig, pool):
    """The copy to the host, then the module's numpy path image by image on the pool's threads."""
    from uaps_amd import InstanceResult, match_instances
    t0 = time.perf_counter()
    hp, hg = [t.cpu() for t in ip[:3]], [t.cpu() for t in ig[:3]]
    t1 = time.perf_counter()
    one = lambda b: match_instances(InstanceResult(*[t[b:b + 1] for t in hp]), InstanceResult(*[t[b:b + 1] for t in hg]), C, iou_threshold=THR)
    res = list(pool.map(one, range(B)))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uaps_amd import label_instances, match_instances
    dev = torch.device("cuda:0")
    res = {"batch": B, "H": H, "W": W, "classes": C, "max_instances": M, "connectivity": 8, "iou_threshold": THR, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "host_threads": 16, "pair_matrix_bytes": B * M * M * 4, "fillings": {}}
    whole = torch.empty((B, M, M), dtype=torch.int32, device=dev)
    res["zero_whole_matrix_us_median"] = statistics.median(call_us(lambda: whole.zero_(), a.reps))
    fill = fillings()
    preds = predictions(fill)
    with ThreadPoolExecutor(16) as pool:
        for name, gt in fill.items():
            ip = label_instances(torch.from_numpy(preds[name]).to(dev), connectivity=8, max_instances=M)
            ig = label_instances(torch.from_numpy(gt).to(dev), connectivity=8, max_instances=M)
            fn = lambda: match_instances(ip, ig, C, iou_threshold=THR)
            comp = lambda: torch_composition(ip, ig)
            r = fn()
            same = all(torch.equal(x, y) for x, y in zip((r.pred, r.target, r.counts), comp()))
            us, us_comp = call_us(fn, a.reps), call_us(comp, a.reps)
            host = [host_today(ip, ig, pool) for _ in range(5)]
            same_host = all(torch.equal(x.cpu(), torch.cat([getattr(h, n) for h in host[0][2]]))
                            for x, n in ((r.pred, "pred"), (r.target, "target"), (r.counts, "counts")))
            res["fillings"][name] = {
                "components_per_image_pred": float(ip.count.float().mean()), "components_per_image_gt": float(ig.count.float().mean()),
                "images_valid": int(r.valid.sum()), "tp": int(r.counts[..., 0].sum()),
                "call_us_median": statistics.median(us), "call_us_min": min(us), "call_us_max": max(us),
                "back_to_back_us": _timed(fn, a.reps) * 1e3, "launches": launch_us(fn, 10),
                "torch_composition_us_median": statistics.median(us_comp), "torch_composition_equal": same,
                "host_copy_us_median": statistics.median(h[0] for h in host), "host_numpy_us_median": statistics.median(h[1] for h in host),
                "host_equal": same_host}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
