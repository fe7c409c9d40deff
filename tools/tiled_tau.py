"""The error table of the tiled-inference kernels (csrc/tiled.hip): per case and window of tests/tiled_ref.py, the fp32 floor (the CPU's
fp32 composition of uaps_amd.tiled against the float64 scatter form), the fold kernel's error against float64 (the Python surface, the
raw entry point with unaligned outputs = the one-pixel form, and the chunked logits) and the bar `TAU` the tests use:
min(1e-4, max(3 x the largest floor, 16 x 2^-24)).  The kernel's own error sets nothing.

    python tools/tiled_tau.py [--out profiles/tiled_forms_tau.txt]          (needs the GPU)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tiled_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uaps_amd import tile_cut, tile_fold, tile_plan
    dev = R.DEV
    lines = [f"Bars of tests/tiled_ref.py over its case table, written by tools/tiled_tau.py on {torch.cuda.get_device_name(0)}.",
             "fp32 floor = the CPU's fp32 composition (uaps_amd.tiled on CPU tensors: softmax per tile, weighted scatter-add, divide) against",
             "the float64 scatter form; kernel = uaps_tile_fold through the Python surface (four-pixel form where W % 4 == 0), through the raw",
             "entry point with outputs at storage offset 1 (one-pixel form), and on logits in chunks of 3 tiles, against float64.  Absolute",
             "errors of probabilities <= 1.", "",
             f"{'case':12s} {'window':>8s} {'C':>2s} {'tiles':>5s} {'fp32 floor':>10s} {'kernel':>10s} {'unaligned':>10s} {'chunked':>10s} {'kernel conf':>11s} {'under margin':>12s}"]
    floor_max = kern_max = 0.0
    for name, kind in R.CASE_WINDOWS:
        case, z_cpu, ref = R.reference(name, kind)
        plan, dims = tile_plan(case.H, case.W, case.tile, case.overlap), (case.B, case.H, case.W)
        floor = float((tile_fold(z_cpu, plan, dims, kind).probs.double() - ref).abs().max())
        z = z_cpu.to(dev)
        res = tile_fold(z, plan, dims, kind)
        ek = float((res.probs.cpu().double() - ref).abs().max())
        ec = float((res.conf.cpu().double() - ref.max(dim=1).values).abs().max())
        ech = float((tile_fold(R.chunked(z), plan, dims, kind).probs.cpu().double() - ref).abs().max())
        pb = torch.zeros(ref.numel() + 1, device=dev)
        wy, wx = (torch.from_numpy(R.window(t, kind).astype(np.float32)).to(dev) for t in case.tile)
        assert R.raw_fold([z], dims, case.tile, case.overlap, wy, wx, pb[1:]) == 0
        eu = float((pb[1:].view(ref.shape).cpu().double() - ref).abs().max())
        under = 1.0 - float(R.clear_pixels(ref).double().mean())
        floor_max, kern_max = max(floor_max, floor), max(kern_max, ek, eu, ech)
        lines.append(f"{case.name:12s} {kind:>8s} {case.C:2d} {z.shape[0]:5d} {floor:10.3e} {ek:10.3e} {eu:10.3e} {ech:10.3e} {ec:11.3e} {under:12.4f}")
    derived = 16 * 2.0 ** -24
    lines += ["", f"largest floor {floor_max:.3e} (3 x = {3 * floor_max:.3e}), derived lower limit 16 x 2^-24 = {derived:.3e}, largest kernel error {kern_max:.3e};",
              f"TAU = min(1e-4, max(3 x floor, 16 x 2^-24)) = {min(1e-4, max(3 * floor_max, derived)):.3e}; tests/tiled_ref.py holds {R.TAU:.3e}"
              f" = {R.TAU / floor_max:.1f} x floor = {R.TAU / kern_max:.1f} x kernel", "",
              "uaps_tile_cut against the numpy-indexed restatement: bit-exact or not (N(0,1) pixels, 3 channels)", ""]
    for case in R.CASES:
        x = torch.randn(case.B, 3, case.H, case.W, generator=torch.Generator().manual_seed(7))
        plan = tile_plan(case.H, case.W, case.tile, case.overlap)
        same = torch.equal(tile_cut(x.to(dev), plan).cpu(), R.cut(x, case.tile, case.overlap))
        lines.append(f"{case.name:12s} {'exact' if same else 'DIFFERS'}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
