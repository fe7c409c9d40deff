"""The error table of the inference-side kernels (tta.hip, tiled.hip, curves.hip): every case of tests/infer_form_cases.py run through the
C ABI as tests/test_gpu_infer_forms.py runs it; per case the form, the kernels it names and, for every float64-compared output, the
largest |got - reference| / bar over its elements (derived per-element bars: must stay <= 1); the other outputs matched bit for bit.

    python tools/infer_tau.py [--out profiles/infer_forms_tau.txt]          (needs the GPU)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import infer_form_cases as E  # noqa: E402
import test_gpu_infer_forms as T  # noqa: E402
from test_bn_ref import kernel_pattern, norm_act_kernel_symbols  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uaps_amd import _lib
    L = _lib.lib()
    rows, worst, failed = [], {}, []
    t0 = time.time()
    for c in E.CASES:
        got, bad, ratios = T.run_case(L, c)
        if bad:
            failed.append((c.id, bad))
        for k, v in ratios.items():
            name = f"{c.entry}.{k}"
            if v > worst.get(name, (-1.0, ""))[0]:
                worst[name] = (v, c.id)
        exact = sorted(k for k in got if k not in ratios)
        form = f"V{c.V}" if c.V else "-"
        rows.append(f"{c.id:24s} {c.entry:9s} {form:3s} " + " ".join(f"{k}={v:.3f}" for k, v in sorted(ratios.items()))
                    + f"  exact: {','.join(exact) or '-'}")
    dt = time.time() - t0
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    head = [f"# tests/test_gpu_infer_forms.py on {torch.cuda.get_device_name(0)} ({arch}): every case of tests/infer_form_cases.py "
            f"({len(E.CASES)} cases, {dt:.1f} s here, references and second launches included)",
            "# (inputs seeded from zlib.crc32 of the case id: the same data in every run)",
            "# each number = max over the output's elements of |got - float64 walk| / bar; the bar of an element is the running error bound of",
            "#   tests/infer_form_cases.py (U = 2^-24 per float32 operation, expf 3 ulp, / 1 ulp, expf(0) exact; x 1.01): must stay <= 1",
            "# exact: matched bit for bit -- the curves' integers and pro_sum (qsum under from_logits: within Q_LOGITS a pixel), the cut, the",
            "#   mask (arg-max of the launch's own probs, and of float64 above twice the bar) and conf (the picked value; TTA: / views)"]
    for k in sorted(worst):
        v, cid = worst[k]
        head.append(f"# largest:  {k} {v:.3f} of its bar ({cid})")
    named = set().union(*(c.kernels for c in E.CASES))
    built = norm_act_kernel_symbols(_lib.LIB_PATH, kernel_pattern(E.KERNEL_NAMES))
    head.append(f"# kernels of tta.hip, tiled.hip, curves.hip in the code object: {len(built)}, named by a case: {len(named & built)}; "
                f"not reached by any case: {', '.join(sorted(built - named)) or 'none'}")
    head.append("# case                     entry     V   error / bar, exact outputs")
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
