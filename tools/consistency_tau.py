"""The error table of the teacher and consistency kernels (loss_mean_teacher.hip, loss_cct_dct.hip, the softmax pairs of pair_ops.hip):
every case of tests/consistency_ref.py run through the C ABI as tests/test_gpu_consistency_forms.py runs it; per case the bit-exact
quantities by name, for every float64-compared quantity the largest |got - reference| / bar (derived bars: must stay <= 1), and the
number of ambiguous mask pixels and clamp-edge draws.

    python tools/consistency_tau.py [--out profiles/consistency_forms_tau.txt]          (needs the GPU)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import consistency_ref as R  # noqa: E402
import test_gpu_consistency_forms as T  # noqa: E402
from test_bn_ref import kernel_pattern, norm_act_kernel_symbols  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tests", default="", help="the count and wall time of tests/test_gpu_consistency_forms.py, for the header")
    a = ap.parse_args()
    from uaps_amd import _lib
    L = _lib.lib()
    L.uaps_set_step_state(None)
    rows, worst, failed = [], {}, []
    t0 = time.time()
    for c in R.CASES:
        ratios, bad, ref = T.run_case(L, c)
        if bad:
            failed.append((c.id, bad))
        for k, v in ratios.items():
            name = f"{c.entry}.{k[:2] if k.startswith('dz') else k}"
            if v > worst.get(name, (-1.0, ""))[0]:
                worst[name] = (v, c.id)
        exact = ",".join(sorted(ref.exact)) or "-"
        if c.entry == "ema":
            exact = f"e0..e{len(ref.exact) - 1}" if len(ref.exact) > 1 else "e0"
        info = " ".join(f"{k}={v}" for k, v in sorted(ref.info.items()) if k in ("ambiguous", "edge"))
        rows.append(f"{c.id:24s} " + " ".join(f"{k}={v:.3e}" for k, v in sorted(ratios.items())) + f"  exact: {exact}" + (f"  {info}" if info else ""))
    dt = time.time() - t0
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    head = [f"# tests/test_gpu_consistency_forms.py on {torch.cuda.get_device_name(0)} ({arch}): every case of tests/consistency_ref.py "
            f"({len(R.CASES)} cases, {dt:.1f} s here, references included)",
            "# (inputs seeded from zlib.crc32 of the case id: the same data in every run)",
            "# exact: the quantities that matched their float32 restatement bit for bit",
            "# each number = max over the case of |got - float64 reference| / bar; the bars are the running error bounds of",
            "#   tests/consistency_ref.py (U = 2^-24 per float32 operation; expf 3, logf 3, sincospif 4, / and sqrtf 1 ulp; __expf 2 U |d| + 1 ulp,",
            "#   __logf 2 ulp + 2 U absolute, rcp 1 ulp; sums (n + 2) U sum|term|): must stay <= 1",
            f"# ambiguous: mask pixels within their bar of the threshold (cap {R.AMBIG_CAP:.0%} of the case); edge: draws within their bar of the clamp",
            f"#   (cap {R.EDGE_CAP:.1%})"]
    for k in sorted(worst):
        v, cid = worst[k]
        head.append(f"# largest:  {k} {v:.3e} ({cid})")
    named = set().union(*(c.kernels for c in R.CASES))
    built = norm_act_kernel_symbols(_lib.LIB_PATH, kernel_pattern(R.KERNEL_NAMES))
    head.append(f"# kernels of the three sources in the code object: {len(built)}, named by a case: {len(named & built)}; "
                f"not reached by any case: {', '.join(sorted(built - named)) or 'none'}")
    if a.tests:
        head.append(f"# tests/test_gpu_consistency_forms.py: {a.tests}")
    head.append("# case                     ratios, exact quantities, counts")
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
