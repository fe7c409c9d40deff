"""Measurements of hysteresis thresholding (csrc/hysteresis.hip, uaps_amd/hysteresis.py), DESIGN.md section 3.33.

Shapes 16 x 4 x 256 x 256 and 2 x 4 x 1024 x 1024 (fp32 probability maps), 8-connectivity, low = 0.25, high = 0.5, every class but
0 selected.  The score maps are built from a label map by the recipe of tests/hysteresis_ref.py (candidates near 0.4, a random 3 % of
them seeds near 0.85, everything else near 0.05), on four fillings:
  sparse   about 10 blobs per image, the realistic case
  noise    class noise at density 0.5: the most components
  full     one component filling every image: every atomic of an image goes to one word
  ring     about 10 annuli per image with salt and pepper
Each case is timed as
  call         events around each of `reps` calls, median and minimum; and back to back (event to event over all calls)
  apply        the apply pass alone (events on its dispatch)
  launches     the median microseconds of every kernel of the call (torch.profiler's kernel records; null where it reports none) and
               their sum per call, "kernels_us_sum"
  composition  the same result composed on the device from what the package had before: torch threshold (max over the selected
               channels, two comparisons, where), label_instances(candidates, maps=(seed,)), a table look-up of the summed seed map
               per component, torch.where.  Its result is asserted equal to the call's.
  host         the device-to-host copy of the scores, then numpy thresholds and scipy.ndimage.label per image and class on 16 threads
Nothing gates on these times.  "algorithmic_bytes" is 4 C + 8 bytes a pixel (the scores read once, the int64 mask written once);
"traffic_bytes" is a MODEL of what the five launches move: scores read and codes written (4 C + 8), codes read and parent and area
words written by the tile pass (16), parents read, roots written and codes read by the flatten pass (at most 16), codes read, root and
area looked up and the mask written by the apply pass (at most 24).  The memory bound the rates are set against is INFERRED from that
model; no hardware counters were collected.

    python tools/bench_hysteresis.py [--reps 50] [--out profiles/hysteresis_bench.json]

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

from _timing import _kernel_ms, _timed  # noqa: E402
from bench_components import fillings  # noqa: E402
from bench_instances import call_us, launch_us  # noqa: E402

C = 4
SHAPES = ((16, 256, 256), (2, 1024, 1024))
LOW, HIGH = 0.25, 0.5
FILLINGS = {"sparse": "sparse", "noise": "noise", "full": "one", "ring": "rings"}        # this tool's names -> bench_components'


def traffic_bytes(N):
    return N * ((4.0 * C + 8.0) + 16.0 + 16.0 + 24.0)


def thresholded(scores):
    """(candidate label map int64 [B,H,W], seed mask bool [B,H,W]) from torch ops."""
    best, k = scores[:, 1:].max(dim=1)
    return torch.where(best >= LOW, k + 1, torch.zeros_like(k)), best >= HIGH


def composed(scores, max_instances):
    """The same mask from what the package had before this entry point, all on the device."""
    from uaps_amd import label_instances
    cand, seed = thresholded(scores)
    zero = torch.zeros_like(cand)
    inst = label_instances(cand, (seed.float(),), max_instances=max_instances)
    seeded = inst.table[:, :, 7] > 0                                        # the summed seed map of every component
    keep = torch.gather(seeded, 1, (inst.labels.long() - 1).clamp_(min=0).flatten(1)).view_as(cand) & (inst.labels > 0)
    return torch.where(keep, cand, zero)


def host_today(scores_dev, pool):
    """What the package's user does without this feature: copy, then numpy and scipy per image (tests/hysteresis_ref.py)."""
    import hysteresis_ref
    t0 = time.perf_counter()
    s = scores_dev.cpu().numpy()
    t1 = time.perf_counter()
    list(pool.map(lambda b: hysteresis_ref.hysteresis(s[b:b + 1], LOW, HIGH), range(s.shape[0])))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))         # the scipy reference and the score recipe of the tests
    import hysteresis_ref
    from uaps_amd import hysteresis, label_instances
    dev = torch.device("cuda:0")
    res = {"classes": C, "connectivity": 8, "low": LOW, "high": HIGH, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "bytes_per_pixel_algorithmic": 4 * C + 8, "host_threads": 16, "counters_collected": False,
           "bound": "memory, inferred from the traffic model of the tool's text", "cases": []}
    with ThreadPoolExecutor(16) as pool:
        for B, H, W in SHAPES:
            N = float(B * H * W)
            labels = fillings(B, H, W)
            for fname, source in FILLINGS.items():
                p, _ = hysteresis_ref.scores_from_labels(labels[source], C)
                scores = torch.from_numpy(p).to(dev)
                fn = lambda: hysteresis(scores, LOW, HIGH)
                out = fn()
                cand = thresholded(scores)[0]
                n_comp = int(label_instances(cand, max_instances=1).count.max())
                M = max(n_comp, 1)                           # a table row for every component: the look-up needs them all
                assert torch.equal(composed(scores, M), out)
                us = call_us(fn, a.reps)
                med = statistics.median(us)
                launches = launch_us(fn, 10)
                ksum = None
                if launches and "error" not in launches:
                    ksum = sum(v["median_us"] * v["launches_per_call"] for v in launches.values())
                comp = lambda: composed(scores, M)
                host = [host_today(scores, pool) for _ in range(3)]
                res["cases"].append({
                    "shape": [B, C, H, W], "filling": fname, "candidate_pixels": int((cand != 0).sum()), "kept_pixels": int((out != 0).sum()),
                    "components_max_per_image": n_comp, "call_us_median": med, "call_us_min": min(us),
                    "back_to_back_us": _timed(fn, a.reps) * 1e3, "apply_kernel_us_mean": _kernel_ms(fn, a.reps) * 1e3,
                    "launches": launches, "kernels_us_sum": ksum, "algorithmic_bytes": (4.0 * C + 8.0) * N,
                    "traffic_bytes": traffic_bytes(N), "GB_s_call_algorithmic": (4.0 * C + 8.0) * N / (med * 1e-6) / 1e9,
                    "GB_s_kernels_traffic": traffic_bytes(N) / (ksum * 1e-6) / 1e9 if ksum else None,
                    "composition_us_median": statistics.median(call_us(comp, a.reps)),
                    "composition_back_to_back_us": _timed(comp, a.reps) * 1e3,
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
