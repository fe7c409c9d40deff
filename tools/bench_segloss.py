"""Measurements of the supervised loss family (csrc/loss_seg.hip) at 16 x 4 x 256 x 256: the time and achieved rate of the forward and
the backward kernel against their algorithmic byte counts (4 C + 8 and 8 C + 8 bytes per pixel) for the {CE, Dice} selection and for
all six terms; forward + backward of all six terms fused against the same terms composed from torch ops (seg_losses.compose, the CPU
path, run on the GPU); and the {CE, Dice} selection against the existing D = 1 supervised loss (uaps_sup_loss), kernel by kernel and
forward + backward.

    python tools/bench_segloss.py [--reps 50] [--repeats 3] [--out file.json]

Prints one JSON object.  Kernel times come from events attached to the kernel's own dispatch (_lib.LaunchTimer), each the mean of
`reps` launches, `repeats` times over (the spread of the repeats is what a difference between two kernels has to exceed).  The working
set (16.8 MB of logits, 8.4 MB of labels) fits in the Infinity Cache: the rates are what the kernels achieve there, not HBM traffic."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from _timing import _kernel_ms, _timed  # noqa: E402


def _profiled_us(fn, names, reps):
    """Mean device time in us of the kernels whose name contains each of `names`, over `reps` calls of `fn` under one kernel trace."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {}
    for n in names:
        ev = [e for e in prof.key_averages() if n in e.key]
        count = sum(e.count for e in ev)
        if count == 0:
            raise RuntimeError(f"the kernel trace holds no {n}")
        out[n] = sum(e.device_time * e.count for e in ev) / count
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import uaps_amd
    from uaps_amd import losses, seg_losses as S
    dev = torch.device("cuda:0")
    B, C, H, W = a.batch, 4, 256, 256
    res = {"batch": B, "classes": C, "H": H, "W": W, "device": torch.cuda.get_device_name(0), "reps": a.reps}
    torch.manual_seed(0)
    z = torch.randn(B, C, H, W, device=dev) * 2
    y = torch.randint(0, C, (B, H, W), device=dev)
    one = torch.ones((), device=dev)
    dz = torch.empty_like(z)
    npix = float(B * H * W)
    fwd_bytes, bwd_bytes = (4 * C + 8) * npix, (8 * C + 8) * npix
    crits = {"ce_dice": S.SegLoss({"ce": 0.5, "dice": 0.5}),
             "all_six": S.SegLoss({k: 1.0 for k in S.TERMS}, class_weight=[1.0, 2.0, 0.5, 1.5], focal_gamma=1.5,
                                  focal_alpha=[0.4, 0.9, 0.7, 0.6], tversky=(0.3, 0.7), dice_sq_weight=[1.0, 0.5, 2.0, 1.5])}

    def rate(ms_list, nbytes):
        ms = sum(ms_list) / len(ms_list)
        return {"us": ms * 1e3, "us_repeats": [m * 1e3 for m in ms_list], "bytes": nbytes, "TB_s": nbytes / (ms * 1e-3) / 1e12}
    res["kernels"] = {}
    for name, crit in crits.items():
        prm = crit.spec.cparams(C)
        scalars = S._fwd(prm, z, y)
        res["kernels"][name + "_fwd"] = rate([_kernel_ms(lambda: S._fwd(prm, z, y), a.reps) for _ in range(a.repeats)], fwd_bytes)
        res["kernels"][name + "_bwd"] = rate([_kernel_ms(lambda: S._bwd(prm, z, y, scalars, one, dz), a.reps) for _ in range(a.repeats)],
                                             bwd_bytes)

    # {CE, Dice} against the existing D = 1 supervised loss (0.5 (CE + Dice)) on the same tensors, kernel by kernel.  uaps_sup_fwd /
    # uaps_sup_bwd do not take launch events on their dispatch, so both sides are read from one kernel trace (torch.profiler: the
    # device time of each kernel by name), the same method for old and new
    zs = z.clone().requires_grad_(True)
    prm = crits["ce_dice"].spec.cparams(C)
    scalars = S._fwd(prm, z, y)

    def both():
        S._fwd(prm, z, y)
        S._bwd(prm, z, y, scalars, one, dz)
        zs.grad = None
        losses.uaps_sup_loss((zs,), y).loss.backward()
    names = ("seg_fwd_kernel", "seg_bwd_kernel", "sup_fwd_kernel", "sup_bwd_kernel")
    traces = [_profiled_us(both, names, a.reps) for _ in range(a.repeats)]
    res["kernel_trace_us"] = {n: {"us": sum(t[n] for t in traces) / len(traces), "us_repeats": [t[n] for t in traces]} for n in names}
    for k in ("fwd", "bwd"):
        res[f"ce_dice_{k}_over_uaps_sup_{k}"] = res["kernel_trace_us"][f"seg_{k}_kernel"]["us"] / res["kernel_trace_us"][f"sup_{k}_kernel"]["us"]

    # forward + backward of a whole criterion
    def fb(fn, leaf):
        def run():
            leaf.grad = None
            fn(leaf).backward()
        return _timed(run, max(3, a.reps // 5))
    zf = z.clone().requires_grad_(True)
    res["all_six_fused_ms"] = fb(lambda t: crits["all_six"](t, y).loss, zf)
    res["all_six_composed_ms"] = fb(lambda t: S.compose(crits["all_six"].spec, t, y)[0], zf)
    res["all_six_composed_over_fused"] = res["all_six_composed_ms"] / res["all_six_fused_ms"]
    res["ce_dice_fused_ms"] = fb(lambda t: crits["ce_dice"](t, y).loss, zf)
    res["uaps_sup_d1_ms"] = fb(lambda t: losses.uaps_sup_loss((t,), y).loss, zf)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
