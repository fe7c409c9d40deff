"""CPS measurements: ms per eager training step of CPSTrainer at 16 + 16 images of 256 x 256, 4 classes (two UNet_f networks), the time
and achieved rate of the two kernels of csrc/loss_cps.hip against their algorithmic byte counts, and the same loss block composed
unfused from existing public pieces -- six D = 1 supervised-loss calls (uaps_sup_loss: 0.5 (CE + Dice)) on the four row windows plus
torch.argmax for the pseudo-labels -- forward + backward, for comparison on the same box.

    python tools/bench_cps.py [--steps 20] [--warmup 5] [--reps 50] [--out file.json]

Prints one JSON object.  Kernel times come from events attached to the kernel's own dispatch (_lib.LaunchTimer); the working set
(2 x 32 x 4 x 256 x 256 floats = 67 MB read, as much again written by the backward) fits in the Infinity Cache, so the rates are what
the kernels achieve there, not HBM traffic."""
import argparse
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
    from uaps_amd import cps, losses
    dev = torch.device("cuda:0")
    B, C, H, W = a.batch, 4, 256, 256
    res = {"batch": B, "classes": C, "H": H, "W": W, "device": torch.cuda.get_device_name(0)}
    data = uaps_amd.data.SyntheticBatches(B, H=H, W=W, device=dev)

    torch.manual_seed(0)
    tr = uaps_amd.CPSTrainer(uaps_amd.net_factory("unet_f", 3, C).to(dev), uaps_amd.net_factory("unet_f", 3, C).to(dev))
    res["cps_step_ms"] = _step_ms(tr, data, a.steps, a.warmup)
    res["images_per_s"] = 2 * B / (res["cps_step_ms"] * 1e-3)
    del tr

    # the kernels on the step's call form: the [2B] logits of the two forward_pair passes
    N = 2 * B
    z1, z2 = torch.randn(N, C, H, W, device=dev) * 2, torch.randn(N, C, H, W, device=dev) * 2
    y = torch.randint(0, C, (B, H, W), device=dev)
    one = torch.ones((), device=dev)
    dz1, dz2 = torch.empty_like(z1), torch.empty_like(z2)
    scalars, _, _ = cps._fwd(z1, z2, y, B)
    logits = 2.0 * N * C * H * W * 4
    k = {"cps_fwd": (_kernel_ms(lambda: cps._fwd(z1, z2, y, B), a.reps), logits + 8.0 * B * H * W + 2.0 * N * H * W),
         "cps_fwd_no_pseudo_store": (_kernel_ms(lambda: cps._fwd(z1, z2, y, B, want_pseudo=False), a.reps), logits + 8.0 * B * H * W),
         "cps_bwd": (_kernel_ms(lambda: cps._bwd(z1, z2, y, B, scalars, one, one, one, dz1, dz2), a.reps), 2 * logits + 8.0 * B * H * W)}
    res["kernels"] = {n: {"us": v[0] * 1e3, "bytes": v[1], "TB_s": v[1] / (v[0] * 1e-3) / 1e12} for n, v in k.items()}

    # the loss block of one step, forward + backward: fused against composed from the D = 1 supervised loss and torch.argmax
    cw = 0.07
    f1, f2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)

    def fused():
        sup, lcps, cp, *_ = cps.cps_loss(f1, f2, y, B)
        f1.grad = f2.grad = None
        (sup + cw * cp + cw * lcps).backward()

    c1, c2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)

    def composed():
        l1, l2, u1, u2 = c1[:B], c2[:B], c1[B:], c2[B:]
        p1, p2 = torch.argmax(c1.detach(), dim=1), torch.argmax(c2.detach(), dim=1)

        def term(z, t):
            return losses.uaps_sup_loss((z,), t).loss
        sup = term(l1, y) + term(l2, y)
        lcps = term(l1, p2[:B]) + term(l2, p1[:B])
        cp = term(u1, p2[B:]) + term(u2, p1[B:])
        c1.grad = c2.grad = None
        (sup + cw * cp + cw * lcps).backward()
    res["fused_loss_block_ms"] = _timed(fused, max(3, a.reps // 5))
    res["composed_loss_block_ms"] = _timed(composed, max(3, a.reps // 5))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
