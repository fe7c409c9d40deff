#!/usr/bin/env python
"""Times the program-interpreting input pipeline (csrc/augment_views.hip) on one MI355X: 16 sources of 200 x 200 x 3 -> 256 x 256.

  arm a  the `neu` recipe through uaps_augment_views against uaps_augment_batch (csrc/augment.hip) on the same draws
  arm b  weak + strong UCC views as one V = 2 launch against two V = 1 launches
  arm c  achieved bytes/s of arm a's new kernel on the algorithmic bytes (sources and masks read once, outputs written once)

Method: both sides of an arm run in this process, alternating, after a warm-up.  One sample = the device-event time of
`--inner` back-to-back launches of a pre-built call (parameters already on the device), divided by `--inner`: the time of a launch
in a stream of launches, i.e. kernel time plus whatever launch gap the queue does not hide.  Medians and quartiles over
`--repeats` samples; the spread of an arm is the inter-quartile range over the median.  Needs the GPU: there is no CPU timing.
Writes profiles/augment_views_bench.json (or --out)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_views_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_augment_views: needs the GPU (no CPU timing exists for these kernels)")
    from uaps_amd import _lib, augment
    from uaps_amd import pipelines as P
    dev = torch.device("cuda:0")
    B, Hs, Ws, Ho, Wo = 16, 200, 200, 256, 256
    rng = np.random.default_rng(0)
    img = torch.from_numpy(rng.integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8)).to(dev)
    mask = torch.from_numpy(rng.integers(0, 4, (B, Hs, Ws), dtype=np.uint8)).to(dev)
    L, stream = _lib.lib(), _lib.current_stream(dev)

    # ---- arm a: one recipe, two kernels, same draws -------------------------------------------------------------------------------
    p = augment.draw_train_params(B, rng)
    rows = P.empty_rows(B)
    for b, (i, f) in enumerate(zip(p.ints, p.floats)):
        rows[b]["hflip"], rows[b]["vflip"], rows[b]["rot_k"] = i[0], i[1], i[2]
        P.set_program(rows[b], [("bc", f[0], f[1])] + ([("blur", int(i[3]))] if i[3] else []) + ([("noise", f[2])] if i[4] else []))
    pi, pf = torch.from_numpy(p.ints).to(dev), torch.from_numpy(p.floats).to(dev)
    x_old = torch.empty((B, 3, Ho, Wo), device=dev)
    y_old = torch.empty((B, Ho, Wo), dtype=torch.int64, device=dev)
    m3, s3 = (C.c_float * 3)(*augment.IMAGENET_MEAN), (C.c_float * 3)(*augment.IMAGENET_STD)

    def old():
        rc = L.uaps_augment_batch(img.data_ptr(), mask.data_ptr(), pi.data_ptr(), pf.data_ptr(), None, 7, B, Hs, Ws, Ho, Wo, m3, s3,
                                  x_old.data_ptr(), y_old.data_ptr(), stream)
        assert rc == 0, rc

    def launcher(draws):
        call, keep, x, y, ws = P._build_call(img, mask, draws, (Ho, Wo), seed=7)
        call.stream = stream
        ref = C.byref(call)

        def go():
            rc = L.uaps_augment_views(ref)
            assert rc == 0, rc
        go.keep = (call, keep, x, y, ws)
        return go

    new = launcher(P.ViewDraws(rows, None, None))
    # ---- arm b: the two UCC views ----------------------------------------------------------------------------------------------
    weak, strong = P.draw("ucc_weak", B, rng), P.draw("ucc_strong", B, rng)
    both, one_w, one_s = launcher([weak, strong]), launcher(weak), launcher(strong)

    def two():
        one_w(); one_s()

    def sample(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.inner           # microseconds per call of fn

    def ab(f, g):
        for _ in range(a.warmup):
            sample(f); sample(g)
        tf, tg = [], []
        for _ in range(a.repeats):                           # alternate: drift and neighbours hit both sides alike
            tf.append(sample(f)); tg.append(sample(g))
        return np.asarray(tf), np.asarray(tg)

    def stats(t):
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        return {"median_us": round(float(med), 3), "q1_us": round(float(q1), 3), "q3_us": round(float(q3), 3),
                "spread": round(float((q3 - q1) / med), 4)}

    t_new, t_old = ab(new, old)
    t_both, t_two = ab(both, two)
    bytes_alg = B * Hs * Ws * 3 + B * Hs * Ws + B * 3 * Ho * Wo * 4 + B * Ho * Wo * 8
    res = {
        "device": torch.cuda.get_device_name(0), "shape": {"B": B, "source": [Hs, Ws, 3], "out": [Ho, Wo]},
        "method": f"device events around {a.inner} back-to-back launches of a pre-built call, per launch; {a.repeats} alternating samples "
                  f"after {a.warmup} warm-up samples; medians, quartiles, spread = IQR / median",
        "arm_a_neu": {"augment_views": stats(t_new), "augment_batch": stats(t_old),
                      "ratio_views_over_batch": round(float(np.median(t_new) / np.median(t_old)), 4),
                      "programs": {"blur": int((p.ints[:, 3] > 0).sum()), "noise": int(p.ints[:, 4].sum())}},
        "arm_b_two_views": {"one_launch_V2": stats(t_both), "two_launches_V1": stats(t_two),
                            "ratio_one_over_two": round(float(np.median(t_both) / np.median(t_two)), 4)},
        "arm_c_bytes": {"algorithmic_bytes": bytes_alg, "what": "sources and masks read once, x and y written once (arm a, augment_views)",
                        "achieved_GBps": round(bytes_alg / (float(np.median(t_new)) * 1e-6) / 1e9, 2)},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
