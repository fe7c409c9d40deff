"""Measurements of the test-time augmentation (csrc/tta.hip, uaps_amd/tta.py) at the workload's shape, 16 x 3 x 256 x 256, C = 4, the real
net_factory("unet_uaps", 3, 4), the five default scales:
  kernels        the kernel time of tta_fold and of the five tta_views launches (events on the dispatch) and the achieved bytes/s on their
                 algorithmic bytes (fold: every view's logits read once, the summed map, mask and confidence written once)
  fused/composed the five tta_views + one tta_fold against the torch composition of the same arithmetic on the same logits (resize + flip
                 + cat per scale; softmax, flip, resize, add per view; arg-max and max / views), alternated in one process
  end to end     predict_tta per image against a main-head prediction at scale 1 alone and against the composed-from-torch TTA around the
                 same model (the reference's ten forwards); joined=True (five forwards of 2B) against joined=False (ten of B)

    python tools/bench_tta.py [--reps 20] [--repeats 3] [--out profiles/tta_bench.json]

Prints one JSON object.  Times are means of `reps` calls, `repeats` times over; the spread of the repeats is what a difference has to
exceed.  The views' logits (270 MB) exceed the Infinity Cache: the fold's rate is mostly HBM traffic."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from _timing import _kernel_ms, _timed  # noqa: E402


def _resize(t, size):
    return F.interpolate(t, size=tuple(size), mode="bilinear", align_corners=True)


def composed_views(x, size):
    r = _resize(x, size)
    return torch.cat([r, r.flip(3)])


def composed_fold(zs, size, B):
    acc = None
    for z in zs:
        p = _resize(F.softmax(z[:B], dim=1), size)
        acc = p if acc is None else acc + p
        acc += _resize(F.softmax(z[B:], dim=1).flip(3), size)
    top = acc.max(dim=1)
    return acc, top.indices, top.values / (2 * len(zs))


def composed_tta(model, x, sizes):
    """utilities/base.py:24-46 around the main head: ten forwards of B."""
    acc = None
    for size in sizes:
        cur = _resize(x, size)
        p = _resize(F.softmax(model.forward_main(cur), dim=1), x.shape[-2:])
        acc = p if acc is None else acc + p
        acc += _resize(F.softmax(model.forward_main(cur.flip(3)), dim=1).flip(3), x.shape[-2:])
    return acc.argmax(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import uaps_amd
    from uaps_amd import inference, tta
    dev = torch.device("cuda:0")
    B, Cin, C, H, W = a.batch, 3, 4, 256, 256
    sizes = tta.scaled_sizes(H, W, tta.DEFAULT_SCALES, 16)
    res = {"batch": B, "classes": C, "H": H, "W": W, "sizes": sizes, "device": torch.cuda.get_device_name(0), "reps": a.reps}
    torch.manual_seed(0)
    x = torch.randn(B, Cin, H, W, device=dev)
    zs = [torch.randn(2 * B, C, h, w, device=dev) * 2 for h, w in sizes]

    def rate(ms_list, nbytes):
        ms = sum(ms_list) / len(ms_list)
        return {"us": ms * 1e3, "us_repeats": [m * 1e3 for m in ms_list], "bytes": nbytes, "TB_s": nbytes / (ms * 1e-3) / 1e12}
    o = 4.0 * B * C * H * W
    fold_bytes = sum(4.0 * z.numel() for z in zs) + o + 12.0 * B * H * W
    res["fold_read_over_o"] = sum(4.0 * z.numel() for z in zs) / o
    res["kernels"] = {"tta_fold": rate([_kernel_ms(lambda: tta.tta_fold(zs, (H, W)), a.reps) for _ in range(a.repeats)], fold_bytes)}
    views_ms = [0.0] * a.repeats
    for h, w in sizes:
        ms = [_kernel_ms(lambda: tta.tta_views(x, (h, w)), a.reps) for _ in range(a.repeats)]
        res["kernels"][f"tta_views_{h}x{w}"] = rate(ms, 4.0 * B * Cin * (H * W + 2 * h * w))
        views_ms = [u + v for u, v in zip(views_ms, ms)]
    res["kernels"]["tta_views_all_five"] = rate(views_ms, sum(4.0 * B * Cin * (H * W + 2 * h * w) for h, w in sizes))

    # views + fold against the torch composition of the same arithmetic on the same logits, alternated
    def fused():
        for size in sizes:
            tta.tta_views(x, size)
        tta.tta_fold(zs, (H, W))

    def composed():
        for size in sizes:
            composed_views(x, size)
        composed_fold(zs, (H, W), B)
    got, want = tta.tta_fold(zs, (H, W)), composed_fold(zs, (H, W), B)
    res["fused_minus_composed_max"] = float((got.probs - want[0]).abs().max())
    reps = max(3, a.reps // 2)
    pairs = [(_timed(fused, reps), _timed(composed, reps)) for _ in range(a.repeats)]
    res["views_fold_fused_ms"] = [p[0] for p in pairs]
    res["views_fold_composed_ms"] = [p[1] for p in pairs]
    res["composed_over_fused"] = sum(p[1] for p in pairs) / sum(p[0] for p in pairs)
    res["bytes_ratio_derived"] = 5.9

    # end to end around the real network
    model = uaps_amd.net_factory("unet_uaps", Cin, C).eval()
    reps = max(2, a.reps // 5)
    with torch.no_grad():
        e2e = {"predict_main": [], "predict_tta_joined": [], "predict_tta_two_forwards": [], "composed_tta": []}
        for _ in range(a.repeats):
            e2e["predict_main"].append(_timed(lambda: inference.predict_main(model, x), reps))
            e2e["predict_tta_joined"].append(_timed(lambda: tta.predict_tta(model, x, want=("mask",)), reps))
            e2e["predict_tta_two_forwards"].append(_timed(lambda: tta.predict_tta(model, x, joined=False, want=("mask",)), reps))
            e2e["composed_tta"].append(_timed(lambda: composed_tta(model, x, sizes), reps))
    mean = {k: sum(v) / len(v) for k, v in e2e.items()}
    res["end_to_end_ms_per_image"] = {k: m / B for k, m in mean.items()}
    res["end_to_end_ms_repeats"] = e2e
    res["predict_tta_over_predict_main"] = mean["predict_tta_joined"] / mean["predict_main"]
    res["composed_tta_over_predict_tta"] = mean["composed_tta"] / mean["predict_tta_joined"]
    res["two_forwards_over_joined"] = mean["predict_tta_two_forwards"] / mean["predict_tta_joined"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
