"""Measurements of the binary loss family (csrc/loss_binary.hip) at 16 x 1 x 256 x 256 with int64 labels: the time and achieved rate
of the forward and the backward kernel against their algorithmic byte counts (12 and 16 bytes per pixel) for {bce, fscore} and for all
seven terms; forward + backward through autograd of both selections, fused against the same terms composed from torch ops
(binary_losses.compose, the CPU path, run on the GPU); and, for context, the D = 1 supervised loss (uaps_sup_loss, sup_fwd_kernel /
sup_bwd_kernel) at 16 x 4 x 256 x 256 through autograd.

    python tools/bench_binloss.py [--reps 50] [--repeats 3] [--out profiles/binloss_bench.json]

Prints one JSON object.  Kernel times come from events attached to the kernel's own dispatch (_lib.LaunchTimer), each the mean of
`reps` launches, `repeats` times over.  The working set (4.2 MB of logits, 8.4 MB of labels) fits in the Infinity Cache: the rates are
what the kernels achieve there, not HBM traffic."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from _timing import _kernel_ms, _timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import uaps_amd
    from uaps_amd import _lib, binary_losses as Bn, losses
    dev = torch.device("cuda:0")
    B, H, W = a.batch, 256, 256
    res = {"batch": B, "H": H, "W": W, "device": torch.cuda.get_device_name(0), "reps": a.reps}
    torch.manual_seed(0)
    z = torch.randn(B, 1, H, W, device=dev) * 2
    y = (torch.rand(B, H, W, device=dev) < 0.3).long()
    dz = torch.empty_like(z)
    n_px = B * H * W
    L = _lib.lib()
    need = C.c_size_t()
    _lib.check(L.uaps_binloss_workspace_bytes(B, H, W, C.byref(need)), "uaps_binloss_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    scalars = torch.empty(_lib.BIN_NSCALARS, dtype=torch.float32, device=dev)
    st = _lib.current_stream(dev)
    selections = {"bce_fscore": Bn.BinarySegLoss({"bce": 0.6, "fscore": 0.4}),
                  "all_seven": Bn.BinarySegLoss({k: 1.0 for k in Bn.TERMS}, pos_weight=3.0, tversky=(0.3, 0.7))}
    for name, crit in selections.items():
        prm = crit.spec.cparams(False)

        def fwd():
            _lib.check(L.uaps_binloss_fwd(z.data_ptr(), y.data_ptr(), C.byref(prm), B, H, W, scalars.data_ptr(), ws.data_ptr(), ws.numel(), st), "fwd")

        def bwd():
            _lib.check(L.uaps_binloss_bwd(z.data_ptr(), y.data_ptr(), C.byref(prm), scalars.data_ptr(), None, B, H, W, dz.data_ptr(), st), "bwd")
        for kind, fn, nbytes in (("fwd", fwd, 12.0 * n_px), ("bwd", bwd, 16.0 * n_px)):
            us = [1e3 * _kernel_ms(fn, a.reps) for _ in range(a.repeats)]
            res[f"{name}_{kind}_kernel_us"] = us
            res[f"{name}_{kind}_algorithmic_bytes"] = nbytes
            res[f"{name}_{kind}_gbps"] = nbytes / (min(us) * 1e-6) / 1e9
        zg = z.clone().requires_grad_(True)

        def fused():
            zg.grad = None
            crit(zg, y).loss.backward()

        def composed():
            zg.grad = None
            Bn.compose(crit.spec, zg, y)[0].backward()
        f = [_timed(fused, a.reps) for _ in range(a.repeats)]
        c = [_timed(composed, a.reps) for _ in range(a.repeats)]
        res[f"{name}_fused_fwd_bwd_ms"], res[f"{name}_composed_fwd_bwd_ms"] = f, c
        res[f"{name}_composed_over_fused"] = min(c) / min(f)
    # context: the D = 1 supervised loss {CE, Dice} on four classes, same batch and map
    z4 = (torch.randn(B, 4, H, W, device=dev) * 2).requires_grad_(True)
    y4 = torch.randint(0, 4, (B, H, W), device=dev)

    def sup():
        z4.grad = None
        losses.uaps_sup_loss((z4,), y4).loss.backward()
    res["sup_d1_c4_fwd_bwd_ms"] = [_timed(sup, a.reps) for _ in range(a.repeats)]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
