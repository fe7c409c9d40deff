"""The error table of the binary loss family: per quantity, the fp32 floor (the float64 reference of tests/binloss_ref.py run in
torch.float32 on the CPU) and the kernels' maximum (C ABI, and the Python surface where the case is aligned) over the case table of
the GPU sweep, against the bars `TAU` / `TAU_PAIR` of tests/binloss_ref.py; the same for the sigmoid MSE / KL pair over its shapes.
The rule of the bars (tests/loss_ref.py): about 3x the larger of the two columns.

    python tools/binloss_tau.py [--out profiles/binloss_forms_tau.txt]          (needs the GPU)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import binloss_ref as R  # noqa: E402
import test_gpu_binloss as T  # noqa: E402


def table(rows, tau):
    out = [f"{'quantity':10s} {'fp32 floor':>10s}  {'case':32s} {'kernel max':>10s}  {'case':32s} {'tau':>8s} {'tau/floor':>9s} {'tau/kernel':>10s}"]
    for k, (f, fc, m, mc) in rows.items():
        rf = f"{tau[k] / f:9.1f}" if f else f"{'-':>9s}"
        rm = f"{tau[k] / m:10.1f}" if m else f"{'-':>10s}"
        out.append(f"{k:10s} {f:10.3e}  {fc:32s} {m:10.3e}  {mc:32s} {tau[k]:8.1e} {rf} {rm}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = {k: [0.0, "", 0.0, ""] for k in R.QUANTITIES}
    for case in T.CASES:
        z, t, ref = T._reference(case)
        ef = R.errors(R.reference(case, z, t, dtype=torch.float32), ref)
        ek = R.errors(T.run_c_abi(case, z, t)[0], ref)
        if case.offset == 0:
            ep = R.errors(T.run_python(case, z, t), ref)
            ek = {k: max(ek[k], ep[k]) for k in ek}
        for k in R.QUANTITIES:
            if ef[k] > rows[k][0]:
                rows[k][:2] = [ef[k], case.name]
            if ek[k] > rows[k][2]:
                rows[k][2:] = [ek[k], case.name]
    pair = {k: [0.0, "", 0.0, ""] for k in R.TAU_PAIR}
    for shape, offset in T.PAIR_SHAPES:
        name = "x".join(map(str, shape)) + (f"-off{offset}" if offset else "")
        inputs = T.pair_inputs(shape)
        ef, ek = T.pair_errors(*inputs, T.pair_float32), T.pair_errors(*inputs, T.pair_kernels(offset))
        for k in R.TAU_PAIR:
            if ef[k] > pair[k][0]:
                pair[k][:2] = [ef[k], name]
            if ek[k] > pair[k][2]:
                pair[k][2:] = [ek[k], name]
    lines = [f"Bars of tests/binloss_ref.py over its case table ({len(T.CASES)} cases), written by tools/binloss_tau.py on {torch.cuda.get_device_name(0)}.",
             "fp32 floor = the float64 reference run in torch.float32 on the CPU; kernel max = uaps_binloss_fwd / _bwd through the C ABI and",
             "the Python surface.  Terms and loss relative to max(|ref|, 1e-3), sums relative to n, dz relative to max|dz|.", ""]
    lines += table(rows, R.TAU)
    lines += ["", "The sigmoid MSE / KL pair (TAU_PAIR): the map absolutely, the KL mean relatively, the gradients relative to max|g|.", ""]
    lines += table(pair, R.TAU_PAIR)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
