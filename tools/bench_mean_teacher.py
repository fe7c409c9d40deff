"""Mean Teacher / UAMT measurements: ms per training step of BaselineTrainer, MeanTeacherTrainer and UAMTTrainer at 16 + 16 images of
256 x 256, 4 classes, and the time and achieved bandwidth of the four kernels of csrc/loss_mean_teacher.hip against their
algorithmic byte counts ("Mean Teacher and UAMT"); for comparison the composed path of sibling.py
(uamt_mc_mean_probs + uamt_consistency_loss: T/2 teacher forwards and ATen glue).

    python tools/bench_mean_teacher.py [--steps 20] [--warmup 5] [--reps 50] [--out file.json]

Prints one JSON object.  Kernel times come from events attached to the kernel's own dispatch (the first launch of
ema_update: one for the single-decoder net); the composed / fused consistency paths are event-to-event per call."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


from _timing import _kernel_ms, _step_ms, _timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import uaps_amd
    from uaps_amd import mean_teacher as mt, sibling
    dev = torch.device("cuda:0")
    B, C, H, W, T = a.batch, 4, 256, 256, 8
    res = {"batch": B, "classes": C, "H": H, "W": W, "T": T, "device": torch.cuda.get_device_name(0)}
    data = uaps_amd.data.SyntheticBatches(B, H=H, W=W, device=dev)

    torch.manual_seed(0)
    res["baseline_ms"] = _step_ms(uaps_amd.BaselineTrainer(uaps_amd.UNet(3, C).to(dev)), data, a.steps, a.warmup, False)
    for name, cls in (("mean_teacher_ms", uaps_amd.MeanTeacherTrainer), ("uamt_ms", uaps_amd.UAMTTrainer)):
        stu = uaps_amd.UNet(3, C).to(dev)
        res[name] = _step_ms(cls(stu, copy.deepcopy(stu)), data, a.steps, a.warmup, True)

    # kernels: each timed by events attached to its own dispatch (_lib.LaunchTimer), mean over `reps` calls
    from uaps_amd import _lib
    L, st = _lib.lib(), _lib.current_stream(dev)
    stu, ema = uaps_amd.UNet(3, C).to(dev), uaps_amd.UNet(3, C).to(dev)
    n_par = sum(p.numel() for p in stu.parameters())
    k = {}
    k["ema_update"] = (_kernel_ms(lambda: mt.ema_update(ema, stu, 0.99, 100), a.reps), 12.0 * n_par)
    xu = data.items[0][2]
    k["teacher_noise"] = (_kernel_ms(lambda: mt.teacher_inputs(xu, T), a.reps), 4.0 * (1 + T) * B * 3 * H * W + 4.0 * B * 3 * H * W)
    s = torch.randn(B, C, H, W, device=dev, requires_grad=True)
    e = torch.randn(B, C, H, W, device=dev)
    mc = torch.randn(T * B, C, H, W, device=dev)
    thr = sibling.uamt_threshold(0.05)
    px = B * H * W
    k["mc_consistency_fwd"] = (_kernel_ms(lambda: mt.mc_consistency_full(s.detach(), e, mc, thr, T=T), a.reps), px * ((T + 2) * C * 4 + 1))
    out = mt.mc_consistency_full(s.detach(), e, mc, thr, T=T)
    g, ds = torch.ones((), device=dev), torch.empty_like(s)

    def bwd():
        _lib.check(L.uaps_mc_consistency_bwd(s.data_ptr(), e.data_ptr(), out.mask.data_ptr(), g.data_ptr(), out.sums.data_ptr(), B, C, H, W,
                                             ds.data_ptr(), st), "uaps_mc_consistency_bwd")
    k["mc_consistency_bwd"] = (_kernel_ms(bwd, a.reps), px * (2 * C * 4 + 1 + C * 4))
    res["kernels"] = {n: {"us": v[0] * 1e3, "bytes": v[1], "TB_s": v[1] / (v[0] * 1e-3) / 1e12} for n, v in k.items()}
    res["ema_params"] = n_par

    # composed path (sibling.py): T/2 teacher forwards, softmax / mean with ATen, entropy + pair kernels + ATen mask and sums
    ema.train()

    def composed():
        p = sibling.uamt_mc_mean_probs(ema, xu, C, T)
        return sibling.uamt_consistency_loss(s, e, p, thr)

    def fused_path():
        inp = mt.teacher_inputs(xu, T)
        with torch.no_grad(), uaps_amd.fused.stat_groups(T // 2):
            m = ema(inp[B:])
        return mt.mc_consistency(s, e, m, thr, T=T)
    res["composed_mc_consistency_ms"] = _timed(composed, max(3, a.reps // 10))
    res["fused_mc_consistency_ms"] = _timed(fused_path, max(3, a.reps // 10))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
