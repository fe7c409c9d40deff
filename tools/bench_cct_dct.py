"""CCT / DCT measurements: ms per eager training step of CCTTrainer and DCTTrainer at 16 + 16 images of 256 x 256, 4 classes, the
composed CCT consistency of sibling.py (three softmax_mse_both maps, ATen means, six backward launches) for comparison, and the time and
achieved rate of the kernels of csrc/loss_cct_dct.hip against their algorithmic byte counts.

    python tools/bench_cct_dct.py [--steps 20] [--warmup 5] [--reps 50] [--out file.json]

Prints one JSON object.  Kernel times come from events attached to the kernel's own dispatch (_lib.LaunchTimer); the working sets
fit in the Infinity Cache, so the rates are what the kernels achieve there, not HBM traffic."""
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
    from uaps_amd import _lib, cct_dct, sibling
    dev = torch.device("cuda:0")
    B, C, H, W, D = a.batch, 4, 256, 256, 4
    res = {"batch": B, "classes": C, "H": H, "W": W, "device": torch.cuda.get_device_name(0)}
    data = uaps_amd.data.SyntheticBatches(B, H=H, W=W, device=dev)

    torch.manual_seed(0)
    res["cct_step_ms"] = _step_ms(uaps_amd.CCTTrainer(uaps_amd.net_factory("unet_cct", 3, C).to(dev)), data, a.steps, a.warmup)
    res["dct_step_ms"] = _step_ms(uaps_amd.DCTTrainer(uaps_amd.UNet(3, C).to(dev)), data, a.steps, a.warmup)

    # kernels on the step's call forms: the [2B] logits of forward_pair with the window [B, 2B); the [3B] logits of the grouped DCT forward
    L, st = _lib.lib(), _lib.current_stream(dev)
    heads = [torch.randn(2 * B, C, H, W, device=dev) for _ in range(D)]
    dheads = [torch.empty_like(h) for h in heads]
    one = torch.ones((), device=dev)
    px = B * H * W
    k = {}
    k["cct_consistency_fwd"] = (_kernel_ms(lambda: cct_dct._cct_fwd(heads, B, B), a.reps), 4.0 * px * C * D)
    k["cct_consistency_bwd"] = (_kernel_ms(lambda: cct_dct._cct_bwd(heads, B, B, one, dheads), a.reps), 8.0 * px * C * D)
    xl, _, xu = data.items[0]
    n_in = B * 3 * H * W
    for rot in (0, 1):
        k[f"rot90_batch_k{rot}"] = (_kernel_ms(lambda: cct_dct.rot90_batch(xl, xu, rot), a.reps), 4.0 * 6 * n_in)
    z = torch.randn(3 * B, C, H, W, device=dev)
    dz = torch.empty_like(z)
    for rot in (0, 1):
        k[f"rot_consistency_fwd_k{rot}"] = (_kernel_ms(lambda: cct_dct._rot_fwd(z, 2 * B, z, B, B, rot), a.reps), 8.0 * px * C)
        k[f"rot_consistency_bwd_k{rot}"] = (_kernel_ms(lambda: cct_dct._rot_bwd(z, 2 * B, z, B, B, rot, one, dz, dz), a.reps), 16.0 * px * C)
    res["kernels"] = {n: {"us": v[0] * 1e3, "bytes": v[1], "TB_s": v[1] / (v[0] * 1e-3) / 1e12} for n, v in k.items()}
    del L, st

    # the consistency term of a CCT step, forward + backward: composed (sibling.py) against fused
    hs = [h[B:].clone().requires_grad_(True) for h in heads]

    def composed():
        sibling.cct_consistency_loss(hs[0], hs[1:]).backward()

    hw = [h.clone().requires_grad_(True) for h in heads]

    def fused():
        cct_dct.cct_consistency(hw, B, B).backward()
    res["composed_cct_consistency_ms"] = _timed(composed, max(3, a.reps // 5))
    res["fused_cct_consistency_ms"] = _timed(fused, max(3, a.reps // 5))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
