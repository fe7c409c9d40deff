"""The error table of the kernels between the convolutions (perturbations, up-sampling, joins, Adam): every case of tests/ops_ref.py run
through the C ABI as tests/test_gpu_ops_forms.py runs it; per case the bit-exact quantities by name and, for every float64-compared
quantity, the largest |got - reference| / bar (derived bars: must stay <= 1; Adam: roundings of its conditioning, against
ops_ref.TAU_ADAM = 3x the largest value this table shows).

    python tools/ops_tau.py [--out profiles/ops_forms_tau.txt]          (needs the GPU)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import ops_ref as R  # noqa: E402
import test_gpu_ops_forms as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tests", default="", help="the count and wall time of tests/test_gpu_ops_forms.py, for the header")
    a = ap.parse_args()
    from uaps_amd import _lib
    L = _lib.lib()
    L.uaps_set_step_state(None)
    rows, worst, failed = [], {}, []
    t0 = time.time()
    for c in R.CASES:
        inp = R.inputs(c)
        got, aux, bad = T._launch(L, c, inp)
        ref = R.reference(c, inp, aux=aux)
        ratios, bad2 = R.compare(ref, got)
        if bad or bad2:
            failed.append((c.id, bad + bad2))
        for k, v in ratios.items():
            if v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, c.id)
        exact = ",".join(sorted(ref.exact)) or "-"
        rows.append(f"{c.id:32s} " + " ".join(f"{k}={v:.3e}" for k, v in sorted(ratios.items())) + f"  exact: {exact}")
    dt = time.time() - t0
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    head = [f"# tests/test_gpu_ops_forms.py on {torch.cuda.get_device_name(0)} ({arch}): every case of tests/ops_ref.py ({len(R.CASES)} cases, {dt:.1f} s here), the correct kernels",
            "# (inputs seeded from zlib.crc32 of the case id: the same data in every run)",
            "# exact: the quantities that matched their float32 restatement bit for bit (two NaNs equal whatever their payload)",
            "# each number = max over the case of |got - float64 reference| / bar; att64, out (fan-in), up_part, dlow: the derived bars",
            "#   C 2^-24 mean_c|x|,  (n + 2) 2^-24 sum_k|term_k|,  4 2^-24 sum_corners |w||v|,  16 2^-24 sum |wy||wx||dout|   (must stay <= 1)",
            "# adam_p / adam_m / adam_v: |got - float64 step| / (2^-24 cond), cond = |p| + |update|, |m| + |g|, |v| + g^2 (roundings)"]
    for k in sorted(worst):
        v, cid = worst[k]
        tau = f"  -> TAU_ADAM {k[5:]} {R.TAU_ADAM[k[5:]]} ({R.TAU_ADAM[k[5:]] / v:.1f}x)" if k.startswith("adam_") else "  (bar 1)"
        head.append(f"# largest:  {k} {v:.3e} ({cid}){tau}")
    head.append("# not reached by any case: the 64-bit division of fan_divmod (a tensor of 2^32 float4, 64 GiB)")
    if a.tests:
        head.append(f"# tests/test_gpu_ops_forms.py: {a.tests}")
    head.append("# case                            ratios, exact quantities")
    text = "\n".join(head + rows) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    if failed:
        print("FAILED:", failed)
        sys.exit(1)


if __name__ == "__main__":
    main()
