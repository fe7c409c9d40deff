"""Measurements of the threshold-sweep histograms (csrc/curves.hip, uaps_amd/curves.py) at 16 x 4 x 256 x 256
and 2 x 4 x 1024 x 1024, 1024 bins, the three class rows and the top row, with and without the regions of the ground truth's defects
(about ten blobs per image, max_instances = 256), on three score patterns:
  uniform    every score uniform in [0, 1): the keys of a wave are spread over the bins, nothing to aggregate
  saturated  every score 0 or 1: four keys per row, the wave aggregation's case
  trained    the softmax of logits of scale 6 around the target plus unit noise: nearly every pixel in the first or the last bin

Per case: the median microseconds of one score_curves call (HIP events around each call after a warm-up), the bytes it has to read
and the bandwidth that amounts to, the median per launch (torch.profiler's kernel records; null where it reports none), the same
arithmetic composed from torch ops on the device (bucketise, one bincount per row, the suffix sums per region), and the copy to the
host plus the module's numpy path, the images spread over 16 threads.

    python tools/bench_curves.py [--reps 30] [--out profiles/curves_bench.json]

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

BINS, M, C = 1024, 256, 4
SHAPES = ((16, 256, 256), (2, 1024, 1024))


def targets(B, H, W, seed=0):
    """Background with about ten rectangular defects of classes 1 .. 3 per image."""
    rng = np.random.default_rng(seed)
    t = np.zeros((B, H, W), dtype=np.int64)
    for b in range(B):
        for _ in range(10):
            h, w = rng.integers(H // 32, H // 8, 2)
            y, x = rng.integers(0, H - h), rng.integers(0, W - w)
            t[b, y:y + h, x:x + w] = rng.integers(1, C)
    return t


def scores(pattern, t, seed=1):
    gen = torch.Generator().manual_seed(seed)
    B, H, W = t.shape
    if pattern == "uniform":
        return torch.rand((B, C, H, W), generator=gen)
    if pattern == "saturated":
        return (torch.rand((B, C, H, W), generator=gen) < 0.5).float()
    onehot = torch.nn.functional.one_hot(torch.from_numpy(t), C).permute(0, 3, 1, 2).float()
    return torch.softmax(6.0 * onehot + torch.randn((B, C, H, W), generator=gen), dim=1)


def torch_composition(S, t, reg):
    """hist, and with regions pro_sum and n_regions, of score_curves from torch ops on the device."""
    B, Cn, H, W = S.shape
    idx = (S * float(BINS)).floor().clamp(0, BINS - 1).long()
    base = torch.arange(B, device=S.device)[:, None, None] * (2 * BINS)
    rows = []
    for c in range(1, Cn):
        key = base + (t == c).long() * BINS + idx[:, c]
        rows.append(torch.bincount(key.reshape(-1), minlength=B * 2 * BINS).view(B, 2, BINS))
    top, am = S.max(dim=1)
    key = base + (am == t).long() * BINS + (top * float(BINS)).floor().clamp(0, BINS - 1).long()
    rows.append(torch.bincount(key.reshape(-1), minlength=B * 2 * BINS).view(B, 2, BINS))
    hist = torch.stack(rows, dim=1)
    if reg is None:
        return hist, None, None
    Mg = reg.max_instances
    g = reg.labels.long()
    gi = (g - 1).clamp(0, Mg - 1)
    cls = torch.gather(reg.table[..., 0], 1, gi.reshape(B, -1)).view(B, H, W)
    sc = torch.gather(idx, 1, cls.clamp(0, Cn - 1)[:, None])[:, 0]
    key = (torch.arange(B, device=S.device)[:, None, None] * Mg + gi) * BINS + sc
    key = torch.where(g >= 1, key, torch.full_like(key, B * Mg * BINS))
    rh = torch.bincount(key.reshape(-1), minlength=B * Mg * BINS + 1)[:-1].view(B, Mg, BINS)
    suffix = rh.flip(2).cumsum(2).flip(2).double() / reg.table[..., 1:2].clamp(min=1).double()
    live = torch.arange(Mg, device=S.device)[None] < reg.count.clamp(max=Mg)[:, None]
    of = (reg.table[..., 0][:, None] == torch.arange(1, Cn, device=S.device)[None, :, None]) & live[:, None]      # [B,K,Mg]
    pro = torch.einsum("bkm,bmi->bki", of.double(), suffix)
    return hist, pro, of.sum(2)


def host_today(S, t, reg, pool):
    """The copy to the host, then the module's numpy path image by image on the pool's threads."""
    from uaps_amd import InstanceResult, score_curves
    t0 = time.perf_counter()
    hS, ht = S.cpu(), t.cpu()
    hr = None if reg is None else [v.cpu() for v in reg[:3]]
    t1 = time.perf_counter()
    one = lambda b: score_curves(hS[b:b + 1], ht[b:b + 1], bins=BINS, regions=None if hr is None else InstanceResult(*[v[b:b + 1] for v in hr]))
    res = list(pool.map(one, range(S.shape[0])))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uaps_amd import label_instances, score_curves
    dev = torch.device("cuda:0")
    res = {"bins": BINS, "classes": C, "rows": C, "max_instances": M, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "host_threads": 16, "cases": {}}
    with ThreadPoolExecutor(16) as pool:
        for B, H, W in SHAPES:
            t_np = targets(B, H, W)
            t = torch.from_numpy(t_np).to(dev)
            regions = label_instances(t, max_instances=M)
            for pattern in ("uniform", "saturated", "trained"):
                S = scores(pattern, t_np).to(dev)
                for with_regions in (False, True):
                    reg = regions if with_regions else None
                    for sums in (False, True):
                        fn = lambda: score_curves(S, t, bins=BINS, regions=reg, want_sums=sums)
                        r = fn()
                        us = call_us(fn, a.reps)
                        read = B * H * W * (4 * C + 8 + (4 if with_regions else 0))
                        groups = -(-2 * C // max(1, 65536 // (BINS * (12 if sums else 4))))
                        case = {"call_us_median": statistics.median(us), "call_us_min": min(us), "call_us_max": max(us),
                                "bytes_read_once": read, "row_groups": groups,
                                "GBps_of_one_read": read / statistics.median(us) / 1e3, "launches": launch_us(fn, 5)}
                        if not sums:
                            comp = lambda: torch_composition(S, t, reg)
                            c = comp()
                            case["torch_composition_equal"] = bool(torch.equal(c[0], r.hist)) and (
                                reg is None or (bool(torch.equal(c[2], r.n_regions)) and bool(torch.allclose(c[1], r.pro_sum, rtol=1e-12, atol=0))))
                            case["torch_composition_us_median"] = statistics.median(call_us(comp, max(5, a.reps // 3)))
                            host = [host_today(S, t, reg, pool) for _ in range(3)]
                            case["host_copy_us_median"] = statistics.median(h[0] for h in host)
                            case["host_numpy_us_median"] = statistics.median(h[1] for h in host)
                            case["host_equal"] = bool(torch.equal(r.hist.cpu(), torch.cat([h.hist for h in host[0][2]])))
                        res["cases"][f"{B}x{C}x{H}x{W} {pattern}{' regions' if with_regions else ''}{' sums' if sums else ''}"] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
