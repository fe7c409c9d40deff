"""UCC measurements: ms per eager training step of UCCTrainer at 16 + 16 + 16 images of 256 x 256, 4 classes (net_factory("unet_ucc")),
the time and achieved rate of the three kernels of csrc/loss_ucc.hip against their algorithmic byte counts, and the same input and loss
block composed unfused from existing public pieces -- a torch `where` cut-mix, sibling.ucc_pseudo_supervision and two supervised
ce_loss / dice_loss pairs -- forward + backward, for comparison on the same box.

    python tools/bench_ucc.py [--steps 20] [--warmup 5] [--reps 50] [--out file.json]

Prints one JSON object.  Kernel times come from events attached to the kernel's own dispatch (_lib.LaunchTimer); the working set
(2 x 48 x 4 x 256 x 256 floats = 101 MB read, as much again written by the backward) fits in the Infinity Cache, so the rates are what
the kernels achieve there, not HBM traffic."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


from _timing import _kernel_ms, _timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import uaps_amd
    from uaps_amd import losses, sibling, ucc
    dev = torch.device("cuda:0")
    B, C, H, W = a.batch, 4, 256, 256
    res = {"batch": B, "classes": C, "H": H, "W": W, "device": torch.cuda.get_device_name(0)}
    data = uaps_amd.data.SyntheticBatches(B, H=H, W=W, device=dev)

    torch.manual_seed(0)
    tr = uaps_amd.UCCTrainer(uaps_amd.net_factory("unet_ucc", 3, C).to(dev))

    def step():
        xl, yl, xu = data.next()
        tr.train_step(xl, yl, xu, xu)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    res["ucc_step_ms"] = (time.perf_counter() - t0) * 1e3 / a.steps
    res["images_per_s"] = 3 * B / (res["ucc_step_ms"] * 1e-3)
    del tr

    # the kernels on the step's call form
    x_l, x_wk, x_st = (torch.randn(B, 3, H, W, device=dev) for _ in range(3))
    y = torch.randint(0, C, (B, H, W), device=dev)
    np_rng = np.random.RandomState(0)
    import random
    py_rng = random.Random(0)
    rl, ru = ucc.cutmix_rects(B, H, W, np_rng, py_rng, 0.5), ucc.cutmix_rects(B, H, W, np_rng, py_rng, 0.5)
    N = 3 * B
    z1, z2 = torch.randn(N, C, H, W, device=dev) * 2, torch.randn(N, C, H, W, device=dev) * 2
    one = torch.ones((), device=dev)
    dz1, dz2 = torch.empty_like(z1), torch.empty_like(z2)
    scalars = ucc._fwd(z1, z2, y, B)[0]
    logits = 2.0 * N * C * H * W * 4
    images = 3.0 * B * 3 * H * W * 4
    k = {"ucc_cutmix": (_kernel_ms(lambda: ucc.cutmix_batch(x_l, y, x_wk, x_st, rl, ru), a.reps), 2 * images + 16.0 * B * H * W),
         "ucc_fwd": (_kernel_ms(lambda: ucc._fwd(z1, z2, y, B), a.reps), logits + 8.0 * B * H * W + 2.0 * B * H * W),
         "ucc_fwd_no_pseudo_store": (_kernel_ms(lambda: ucc._fwd(z1, z2, y, B, want_pseudo=False), a.reps), logits + 8.0 * B * H * W),
         "ucc_bwd": (_kernel_ms(lambda: ucc._bwd(z1, z2, y, B, scalars, one, one, dz1, dz2), a.reps), 2 * logits + 8.0 * B * H * W)}
    res["kernels"] = {n: {"us": v[0] * 1e3, "bytes": v[1], "TB_s": v[1] / (v[0] * 1e-3) / 1e12} for n, v in k.items()}

    # the input and the loss block of one step, forward + backward: fused against composed
    cw = 0.07
    f1, f2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)

    def fused():
        _, y_mix = ucc.cutmix_batch(x_l, y, x_wk, x_st, rl, ru)
        sup, ps, *_ = ucc.ucc_loss(f1, f2, y_mix, B)
        f1.grad = f2.grad = None
        (sup + cw * ps).backward()

    c1, c2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    yy, xx = torch.arange(H, device=dev).view(1, H, 1), torch.arange(W, device=dev).view(1, 1, W)

    def masks(r):
        t = torch.tensor(r, device=dev)       # (a host -> device copy per step: what a composed step would do)
        return ((t[:, 0] != 0).view(-1, 1, 1) & (yy >= t[:, 1].view(-1, 1, 1)) & (yy < t[:, 2].view(-1, 1, 1))
                & (xx >= t[:, 3].view(-1, 1, 1)) & (xx < t[:, 4].view(-1, 1, 1)))

    def composed():
        m1, m2 = masks(rl), masks(ru)
        mixed_l = torch.where(m1.unsqueeze(1), torch.roll(x_l, -1, 0), x_l)
        y_mix = torch.where(m1, torch.roll(y, -1, 0), y)
        torch.cat([mixed_l, torch.where(m2.unsqueeze(1), mixed_l, x_wk), torch.where(m2.unsqueeze(1), mixed_l, x_st)])
        sup = 0.5 * (losses.ce_loss(c1[:B], y_mix) + losses.dice_loss(y_mix.unsqueeze(1), c1[:B])) \
            + 0.5 * (losses.ce_loss(c2[:B], y_mix) + losses.dice_loss(y_mix.unsqueeze(1), c2[:B]))
        ps = sibling.ucc_pseudo_supervision(c1[B:2 * B], c2[B:2 * B], c1[2 * B:], c2[2 * B:])[0]
        c1.grad = c2.grad = None
        (sup + cw * ps).backward()
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
