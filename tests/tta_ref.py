"""Float64 restatement of the test-time augmentation (utilities/base.py:24-46) for tests/test_tta_host.py, tests/test_gpu_tta.py and
tools/tta_tau.py: the torch composition in a chosen dtype, the explicit gather form of include/uaps_hip.h ("Test-time augmentation"),
the case table of the GPU sweep with its cached references, the raw entry-point call both use, and the bars.

The bars: a kernel evaluates the same formulas in fp32 in a different but equally valid order (fused multiply-adds, another expf), so
its error against float64 is of the size of the fp32 torch composition's own -- the floor -- and not below it.  As for the binary
losses (tests/binloss_ref.py) the bar is 3x the floor, capped at the project's 1e-4 contract.  The floors are those of the CPU's fp32
composition over CASES / VIEW_SHAPES x VIEW_SIZES (tools/tta_tau.py prints them beside the kernels' errors, profiles/tta_forms_tau.txt):
    summed map   1.87e-5 (the saturated case with flip; 1.28e-5 on N(0, 2^2) logits)   -> TAU_SUM   = 5.6e-5
    resized view 1.36e-5 (N(0,1) pixels resized 32x48 -> 48x72)                         -> TAU_VIEWS = 4.1e-5
Both floors are mostly the fp32 source coordinate r * dst (r rounded to a float, times an index of up to 95), which a kernel that
follows torch's formula shares; the rest is the order of the fp32 sums.
conf = max / views carries 1 / views of the summed map's error and is held to TAU_SUM as well."""
import ctypes as C
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

DEFAULT_SCALES = (0.5, 0.75, 1.0, 1.5, 2.0)
TAU_SUM = 5.6e-5
TAU_VIEWS = 4.1e-5
MARGIN = 1e-4            # the float64 top-2 margin above which the arg-max must agree
DEV = "cuda:0"
MAX_EXCLUDED = 0.01      # at most this share of the pixels may fall under MARGIN

Case = namedtuple("Case", "name B C H W sizes gain")


def _int_sizes(H, W, scales):
    return tuple((int(H * s), int(W * s)) for s in scales)


CASES = (
    Case("odd-17x23", 1, 8, 17, 23, _int_sizes(17, 23, DEFAULT_SCALES), 2.0),
    Case("vec-32x48", 2, 4, 32, 48, _int_sizes(32, 48, DEFAULT_SCALES), 2.0),
    Case("c7-24x40", 2, 7, 24, 40, _int_sizes(24, 40, (0.5, 1.0, 1.5)), 2.0),
    Case("s8-16x16", 1, 2, 16, 16, ((8, 8), (12, 20), (16, 16), (24, 24), (32, 32), (48, 48), (1, 16), (16, 1)), 2.0),
    Case("one-pixel", 1, 3, 1, 1, ((4, 4),), 2.0),
    Case("saturated", 2, 4, 32, 48, _int_sizes(32, 48, DEFAULT_SCALES), 60.0),      # N(0, 2^2) x 30
)
VIEW_SHAPES = ((2, 3, 32, 48), (1, 1, 17, 23))
VIEW_SIZES = ((16, 24), (24, 36), (48, 72), (64, 96), (8, 11), (1, 5))


def case_logits(case, flip):
    """Seeded logits ~ N(0, gain^2), one tensor [(2 if flip else 1) * B, C, h, w] per scale (CPU, fp32)."""
    gen = torch.Generator().manual_seed(1000 + sum(map(ord, case.name)))
    n = (2 if flip else 1) * case.B
    return [torch.randn(n, case.C, h, w, generator=gen) * case.gain for h, w in case.sizes]


def resize(t, size):
    return F.interpolate(t, size=tuple(size), mode="bilinear", align_corners=True)


def views(x, size, flip=True, dtype=torch.float64):
    r = resize(x.to(dtype), size)
    return torch.cat([r, r.flip(3)]) if flip else r


def fold(logits_list, out_size, flip=True, dtype=torch.float64):
    """The reference's loop on the views' logits, in its order: the summed map [B,C,H,W] in `dtype`."""
    B = logits_list[0].shape[0] // (2 if flip else 1)
    acc = None
    for z in logits_list:
        z = z.to(dtype)
        p = resize(F.softmax(z[:B], dim=1), out_size)
        acc = p if acc is None else acc + p
        if flip:
            acc = acc + resize(F.softmax(z[B:], dim=1).flip(3), out_size)
    return acc


def _corners(n_in, n_out, dtype):
    r = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    src = torch.arange(n_out, dtype=dtype) * r
    i0 = src.floor().long().clamp_(max=n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = src - i0.to(dtype)
    return i0, i1, l1


def fold_gather(logits_list, out_size, flip=True, dtype=torch.float64):
    """The explicit gather form the kernel implements: softmax at the four source corners, the flipped half read at the mirrored
    columns w - 1 - x0 / w - 1 - x1 of image B + b, value = l0h (l0w v00 + l1w v01) + l1h (l0w v10 + l1w v11)."""
    H, W = out_size
    B = logits_list[0].shape[0] // (2 if flip else 1)
    acc = None
    for z in logits_list:
        p = F.softmax(z.to(dtype), dim=1)
        h, w = p.shape[2:]
        y0, y1, ly = _corners(h, H, dtype)
        x0, x1, lx = _corners(w, W, dtype)
        ly, lx = ly[:, None], lx[None, :]
        for half in range(2 if flip else 1):
            q = p[half * B:(half + 1) * B]
            c0, c1 = (x0, x1) if half == 0 else (w - 1 - x0, w - 1 - x1)
            v00, v01 = q[:, :, y0][:, :, :, c0], q[:, :, y0][:, :, :, c1]
            v10, v11 = q[:, :, y1][:, :, :, c0], q[:, :, y1][:, :, :, c1]
            t = (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11)
            acc = t if acc is None else acc + t
    return acc


def clear_pixels(ref_sum, margin=MARGIN):
    """[B,H,W] bool: the float64 top-2 margin exceeds `margin`."""
    top2 = ref_sum.topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) > margin


def check_mask(mask, ref_sum):
    """mask == the float64 arg-max wherever the float64 top-2 margin exceeds MARGIN; at most MAX_EXCLUDED of the pixels fall under it."""
    clear = clear_pixels(ref_sum)
    excluded = 1.0 - float(clear.double().mean())
    assert excluded <= MAX_EXCLUDED, f"{excluded:.4f} of the pixels under the margin"
    want = ref_sum.argmax(dim=1)
    assert torch.equal(mask.cpu()[clear], want[clear])


@functools.lru_cache(maxsize=None)
def reference(name, flip):
    """(CPU logits, float64 summed map) of a case: computed once, shared, never written."""
    case = next(c for c in CASES if c.name == name)
    zs = case_logits(case, flip)
    return case, zs, fold(zs, (case.H, case.W), flip)


def raw_fold(zs, dims, flip, probs=None, mask=None, conf=None, struct=None, over=None):
    """uaps_tta_fold through the raw entry point; dims = (B, H, W); `over` replaces fields (S, C, ..., struct_size) after they are filled in."""
    from uaps_amd import _lib
    call = struct if struct is not None else _lib.TTAFoldCall()
    base = call.base if struct is not None else call
    base.struct_size = C.sizeof(call)
    base.S, (base.B, base.H, base.W), base.C, base.flip = len(zs), dims, zs[0].shape[1], int(flip)
    for s, z in enumerate(zs):
        base.logits[s], base.h[s], base.w[s] = z.data_ptr(), z.shape[2], z.shape[3]
    base.probs_sum = probs.data_ptr() if probs is not None else None
    base.mask = mask.data_ptr() if mask is not None else None
    base.conf = conf.data_ptr() if conf is not None else None
    base.stream = _lib.current_stream(zs[0].device)
    for k, v in (over or {}).items():
        if k.startswith("logits") or k[0] in "hw" and k[1:].isdigit():
            getattr(base, k.rstrip("0123456789"))[int(k[-1])] = v
        else:
            setattr(base, k, v)
    return _lib.lib().uaps_tta_fold(C.byref(call))
