"""The error table of the test-time augmentation kernels (csrc/tta.hip): per case of tests/tta_ref.py, the fp32 floor (the float64
restatement run in torch.float32 on the CPU), the kernels' error against float64 (the Python surface, and the raw entry point with
unaligned outputs = the one-pixel form) and the bars `TAU_SUM` / `TAU_VIEWS` the tests use: 3x the largest floor, capped at 1e-4.

    python tools/tta_tau.py [--out profiles/tta_forms_tau.txt]          (needs the GPU)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import tta_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uaps_amd import tta_fold, tta_views
    dev = R.DEV
    lines = [f"Bars of tests/tta_ref.py over its case table, written by tools/tta_tau.py on {torch.cuda.get_device_name(0)}.",
             "fp32 floor = the torch composition (utilities/base.py:24-46 on the views' logits) in torch.float32 on the CPU against the same",
             "in float64; kernel = uaps_tta_fold through the Python surface (four-pixel form where W % 4 == 0) and through the raw entry",
             "point with outputs at storage offset 1 (one-pixel form), against float64.  Absolute errors; the summed map reaches 10.", "",
             f"{'case':12s} {'flip':>4s} {'S':>2s} {'C':>2s} {'fp32 floor':>10s} {'kernel sum':>10s} {'unaligned':>10s} {'kernel conf':>11s} {'under margin':>12s}"]
    floor_max = kern_max = 0.0
    for case in R.CASES:
        for flip in (True, False):
            _, zs_cpu, ref = R.reference(case.name, flip)
            size, views = (case.H, case.W), len(zs_cpu) * (2 if flip else 1)
            floor = float((R.fold(zs_cpu, size, flip, torch.float32).double() - ref).abs().max())
            zs = [z.to(dev) for z in zs_cpu]
            res = tta_fold(zs, size, flip)
            ek = float((res.probs.cpu().double() - ref).abs().max())
            ec = float((res.conf.cpu().double() - ref.max(dim=1).values / views).abs().max())
            pb = torch.zeros(ref.numel() + 1, device=dev)
            assert R.raw_fold(zs, (case.B, case.H, case.W), flip, pb[1:]) == 0
            eu = float((pb[1:].view(ref.shape).cpu().double() - ref).abs().max())
            under = 1.0 - float(R.clear_pixels(ref).double().mean())
            floor_max, kern_max = max(floor_max, floor), max(kern_max, ek, eu)
            lines.append(f"{case.name:12s} {int(flip):4d} {len(zs):2d} {case.C:2d} {floor:10.3e} {ek:10.3e} {eu:10.3e} {ec:11.3e} {under:12.4f}")
    lines += ["", f"largest floor {floor_max:.3e}, largest kernel error {kern_max:.3e}; TAU_SUM = {R.TAU_SUM:.1e} = min(1e-4, 3 x floor)"
              f" = {R.TAU_SUM / floor_max:.1f} x floor = {R.TAU_SUM / kern_max:.1f} x kernel", "",
              "uaps_tta_views against the float64 resize (N(0,1) pixels), both halves:", "",
              f"{'source':14s} {'size':>9s} {'fp32 floor':>10s} {'kernel':>10s}"]
    vfloor = vkern = 0.0
    for shape in R.VIEW_SHAPES:
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(5))
        for size in R.VIEW_SIZES:
            ref = R.views(x, size)
            floor = float((R.views(x, size, True, torch.float32).double() - ref).abs().max())
            ek = float((tta_views(x.to(dev), size).cpu().double() - ref).abs().max())
            vfloor, vkern = max(vfloor, floor), max(vkern, ek)
            lines.append(f"{'x'.join(map(str, shape)):14s} {'x'.join(map(str, size)):>9s} {floor:10.3e} {ek:10.3e}")
    lines += ["", f"largest floor {vfloor:.3e}, largest kernel error {vkern:.3e}; TAU_VIEWS = {R.TAU_VIEWS:.1e} = min(1e-4, 3 x floor)"
              f" = {R.TAU_VIEWS / vfloor:.1f} x floor = {R.TAU_VIEWS / vkern:.1f} x kernel"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
