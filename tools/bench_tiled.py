"""Measurements of tiled full-resolution inference (csrc/tiled.hip, uaps_amd/tiled.py): 2 x 3 x 1024 x 1024, C = 4, tile 256, overlap 32,
triangle window -- 5 x 5 tiles per image, 50 tiles, 1.56x the image's pixels:
  kernels        the kernel time of tile_cut and tile_fold (events on the dispatch) and the achieved bytes/s on their algorithmic bytes
                 (uaps_account: every tile element read once, every output written once)
  fused/composed tile_cut + tile_fold against the same arithmetic composed from torch ops on the same logits (index the tiles out, softmax,
                 weighted scatter-add per tile position, a second accumulator for the weights, divide, arg-max), alternated in one process
  end to end     predict_tiled per megapixel next to predict_main on the same images run whole (the network is fully convolutional: this
                 prices the overlap's redundant pixels and the tiles' smaller launches)

    python tools/bench_tiled.py [--reps 20] [--repeats 3] [--out profiles/tiled_bench.json]

Prints one JSON object.  Times are means of `reps` calls, `repeats` times over; "us" / "ms" are the medians of the repeats and the spread
of the repeats is what a difference has to exceed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from _timing import _kernel_ms, _timed  # noqa: E402


def composed_cut(x, plan):
    th, tw = plan.tile
    return torch.stack([x[b, :, y0:y0 + th, x0:x0 + tw] for b in range(x.shape[0]) for y0 in plan.ys for x0 in plan.xs])


def composed_fold(z, plan, B, H, W, w2):
    """softmax, weighted scatter-add per tile position (all images at once), the weights' accumulator, divide, arg-max."""
    th, tw = plan.tile
    ny, nx = len(plan.ys), len(plan.xs)
    p = F.softmax(z, dim=1).view(B, ny, nx, z.shape[1], th, tw) * w2
    acc = torch.zeros(B, z.shape[1], H, W, device=z.device)
    norm = torch.zeros(H, W, device=z.device)
    for iy, y0 in enumerate(plan.ys):
        for ix, x0 in enumerate(plan.xs):
            acc[:, :, y0:y0 + th, x0:x0 + tw] += p[:, iy, ix]
            norm[y0:y0 + th, x0:x0 + tw] += w2
    probs = acc / norm
    top = probs.max(dim=1)
    return probs, top.indices, top.values


def accounted(fn):
    from uaps_amd import _lib
    L = _lib.lib()
    L.uaps_account(1)
    before = L.uaps_accounted_bytes()
    fn()
    after = L.uaps_accounted_bytes()
    L.uaps_account(0)
    return after - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import uaps_amd
    from uaps_amd import inference, tiled
    dev = torch.device("cuda:0")
    B, Cin, C, H, W, tile, overlap = 2, 3, 4, a.size, a.size, 256, 32
    plan = tiled.tile_plan(H, W, tile, overlap)
    total = B * len(plan.ys) * len(plan.xs)
    res = {"batch": B, "classes": C, "H": H, "W": W, "tile": tile, "overlap": overlap, "window": "triangle", "tiles": total,
           "tile_pixels_over_image_pixels": total * tile * tile / (B * H * W), "device": torch.cuda.get_device_name(0), "reps": a.reps}
    torch.manual_seed(0)
    x = torch.randn(B, Cin, H, W, device=dev)
    z = torch.randn(total, C, tile, tile, device=dev) * 2

    def rate(ms_list, nbytes):
        ms = statistics.median(ms_list)
        return {"us": ms * 1e3, "us_repeats": [m * 1e3 for m in ms_list], "bytes": nbytes, "TB_s": nbytes / (ms * 1e-3) / 1e12}
    cut_bytes = accounted(lambda: tiled.tile_cut(x, plan))
    fold_bytes = accounted(lambda: tiled.tile_fold(z, plan, (B, H, W)))
    mask_bytes = accounted(lambda: tiled.tile_fold(z, plan, (B, H, W), want=("mask",)))
    res["kernels"] = {
        "tile_cut": rate([_kernel_ms(lambda: tiled.tile_cut(x, plan), a.reps) for _ in range(a.repeats)], cut_bytes),
        "tile_fold": rate([_kernel_ms(lambda: tiled.tile_fold(z, plan, (B, H, W)), a.reps) for _ in range(a.repeats)], fold_bytes),
        "tile_fold_mask_only": rate([_kernel_ms(lambda: tiled.tile_fold(z, plan, (B, H, W), want=("mask",)), a.reps) for _ in range(a.repeats)],
                                    mask_bytes)}

    # cut + fold against the torch composition of the same arithmetic on the same logits, alternated
    w1 = tiled.tile_window(tile, "triangle").to(dev)
    w2 = w1[:, None] * w1[None, :]

    def fused():
        tiled.tile_cut(x, plan)
        tiled.tile_fold(z, plan, (B, H, W))

    def composed():
        composed_cut(x, plan)
        composed_fold(z, plan, B, H, W, w2)
    got, want = tiled.tile_fold(z, plan, (B, H, W)), composed_fold(z, plan, B, H, W, w2)
    res["fused_minus_composed_max"] = float((got.probs - want[0]).abs().max())
    res["cut_equal_composed"] = bool(torch.equal(tiled.tile_cut(x, plan), composed_cut(x, plan)))
    reps = max(3, a.reps // 2)
    pairs = [(_timed(fused, reps), _timed(composed, reps)) for _ in range(a.repeats)]
    res["cut_fold_fused_ms"] = [p[0] for p in pairs]
    res["cut_fold_composed_ms"] = [p[1] for p in pairs]
    res["composed_over_fused"] = statistics.median(p[1] for p in pairs) / statistics.median(p[0] for p in pairs)

    # end to end around the real network
    model = uaps_amd.net_factory("unet_uaps", Cin, C).eval()
    reps = max(2, a.reps // 5)
    mpix = B * H * W / 1e6
    with torch.no_grad():
        e2e = {"predict_main_whole": [], "predict_tiled": [], "predict_tiled_batch_tiles_10": []}
        for _ in range(a.repeats):
            e2e["predict_main_whole"].append(_timed(lambda: inference.predict_main(model, x), reps))
            e2e["predict_tiled"].append(_timed(lambda: tiled.predict_tiled(model, x, tile, overlap, want=("mask",)), reps))
            e2e["predict_tiled_batch_tiles_10"].append(_timed(lambda: tiled.predict_tiled(model, x, tile, overlap, batch_tiles=10, want=("mask",)), reps))
        whole = inference.predict_main(model, x)
        agree = float((tiled.predict_tiled(model, x, tile, overlap, want=("mask",)).mask == whole).float().mean())
    med = {k: statistics.median(v) for k, v in e2e.items()}
    res["end_to_end_ms_per_megapixel"] = {k: m / mpix for k, m in med.items()}
    res["end_to_end_ms_repeats"] = e2e
    res["predict_tiled_over_predict_main_whole"] = med["predict_tiled"] / med["predict_main_whole"]
    res["tiled_mask_agrees_with_whole"] = agree
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
