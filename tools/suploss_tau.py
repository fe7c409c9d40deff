"""The error table of the CPS, UCC (cut-mix included) and supervised-loss kernels (loss_cps.hip, loss_ucc.hip, loss_seg.hip): every case
of tests/suploss_ref.py run through the C ABI as tests/test_gpu_suploss_forms.py runs it; per case the bit-exact quantities by name and,
for every float64-compared quantity, the largest |got - reference| / bar (derived bars: must stay <= 1); the label-edge rows; the kernels
built, named and not reached.

    python tools/suploss_tau.py [--out profiles/suploss_forms_tau.txt]          (needs the GPU)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import binloss_ref as Bn  # noqa: E402
import suploss_ref as R  # noqa: E402
import test_gpu_suploss_forms as T  # noqa: E402
from test_bn_ref import kernel_pattern, norm_act_kernel_symbols  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tests", default="", help="the count and wall time of tests/test_gpu_suploss_forms.py, for the header")
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
            name = f"{c.entry}.{k}"
            if v > worst.get(name, (-1.0, ""))[0]:
                worst[name] = (v, c.id)
        form = f"V{c.V()}" if c.entry == "cutmix" else f"V{c.V('fwd')}/V{c.V('bwd')}"
        rows.append(f"{c.id:22s} {form:6s} " + " ".join(f"{k}={v:.3e}" for k, v in sorted(ratios.items())) + f"  exact: {','.join(sorted(ref.exact)) or '-'}")
    dt = time.time() - t0
    edges = []
    for name, run in T.EDGES:
        x, y, n, bad_a, bad_b = run(L)
        differ = [k for k in x if x[k] is not None and not T._same(x[k], y[k])]
        edges.append(f"# label edges {name:16s} planted {n:2d} counted {bad_a:.0f} outputs that differ from the -1 run: {', '.join(differ) or 'none'}")
        if differ or bad_a != n or bad_b != n:
            failed.append((name, differ, bad_a, n))
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    head = [f"# tests/test_gpu_suploss_forms.py on {torch.cuda.get_device_name(0)} ({arch}): every case of tests/suploss_ref.py "
            f"({len(R.CASES)} cases, {dt:.1f} s here, references and second launches included)",
            "# (inputs seeded from zlib.crc32 of the case id: the same data in every run)",
            "# exact: the quantities that matched bit for bit (pseudo-label bytes, the out-of-range count, reserved scalars, cut-mix outputs,",
            "#   mixed labels and max|.|, the variance maps of two identical heads, seg's counts)",
            "# each number = max over the case of |got - float64 reference| / bar; the bars are the running error bounds of tests/suploss_ref.py",
            "#   (U = 2^-24 per float32 operation; expf 3, logf 3, / 1 ulp; sums (n + 2) U sum|term|, n = trips x V + 8; the finalize in double,",
            "#   bounded as float32): must stay <= 1.  Every bar is below 2^-10 of its tensor's largest |value| (asserted before each launch)."]
    for k in sorted(worst):
        v, cid = worst[k]
        head.append(f"# largest:  {k} {v:.3e} ({cid})")
    head += edges
    named = set().union(*(c.kernels for c in R.CASES)) | R.seg_sweep_kernels()
    built = norm_act_kernel_symbols(_lib.LIB_PATH, kernel_pattern(R.KERNEL_NAMES))
    own = set().union(*(c.kernels for c in R.CASES))
    head.append(f"# kernels of loss_cps.hip, loss_ucc.hip, loss_seg.hip in the code object: {len(built)}, named by a case: {len(named & built)} "
                f"({len(own & built)} by this table, the rest by the sweep of tests/test_gpu_seglosses.py); "
                f"not reached by any case: {', '.join(sorted(built - named)) or 'none'}")
    built_bin = norm_act_kernel_symbols(_lib.LIB_PATH, kernel_pattern(Bn.KERNEL_NAMES))
    named_bin = set().union(*(c.kernels for c in Bn.CASES)) | Bn.PAIR_KERNELS | Bn.CONFUSION_KERNELS
    head.append(f"# kernels of loss_binary.hip in the code object: {len(built_bin)}, named by tests/binloss_ref.py: {len(named_bin & built_bin)}; "
                f"not reached by any case: {', '.join(sorted(built_bin - named_bin)) or 'none'}")
    if a.tests:
        head.append(f"# tests/test_gpu_suploss_forms.py: {a.tests}")
    head.append("# case                   fwd/bwd ratios, exact quantities")
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
