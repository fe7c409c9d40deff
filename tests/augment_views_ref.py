"""Numpy restatement of the program interpreter of csrc/augment_views.hip (include/uaps_hip.h, uaps_augment_views).
TEST INFRASTRUCTURE, NOT PRODUCT.  PARITY UNPINNED: this restates the arithmetic the header writes down, not cv2 / albumentations.

It works STAGE BY STAGE ON WHOLE IMAGES -- resize, flips, quarter turns, then one array operation per op of the program, with a
uint8 image between the stages -- so its structure shares nothing with the gather kernel (which evaluates a pixel's whole history
at once: corners, taps, segments).  The contrast mean is taken from the actual intermediate image.

`ft` is the float type of the inexact stages (bilinear weights, v * f, HSV): float64 is the reference the kernel is held to, float32
is used only to measure how often float32 rounding alone moves a value across a rounding tie (see `cases`).
"""
import numpy as np

from uaps_amd import _lib
from uaps_amd import pipelines as P


def resize_nearest(img, Ho, Wo):
    Hs, Ws = img.shape[:2]
    ys = np.minimum((np.arange(Ho) * Hs) // Ho, Hs - 1)
    xs = np.minimum((np.arange(Wo) * Ws) // Wo, Ws - 1)
    return img[ys][:, xs]


def _trunc_u8(t):
    return np.clip(t, 0, 255).astype(np.uint8)            # astype truncates, as the uint8 LUTs do


def _rint_u8(t):
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def box_blur(img, k):
    r = k // 2
    p = np.pad(img.astype(np.int64), ((r, r), (r, r), (0, 0)), mode="reflect")        # numpy 'reflect' == BORDER_REFLECT_101
    H, W = img.shape[:2]
    acc = np.zeros(img.shape, np.int64)
    for dy in range(k):
        for dx in range(k):
            acc += p[dy:dy + H, dx:dx + W]
    return np.rint(acc / float(k * k)).astype(np.uint8)   # k * k is odd: no sum lies on a tie


def _nodes(pos, n):
    pos = np.clip(pos.astype(np.float32), 0, n - 1)
    i0 = np.floor(pos).astype(np.int64)
    i1 = i0 + 1
    i1 = np.where(i1 >= n, 2 * (n - 1) - i1, i1) if n > 1 else np.zeros_like(i1)
    return i0, i1, pos - np.floor(pos)


def grid_sample(img, gys, gxs, ft):
    H, W = img.shape[:2]
    y0, y1, wy = _nodes(gys, H)
    x0, x1, wx = _nodes(gxs, W)
    f = img.astype(ft)
    wy, wx = wy.astype(ft)[:, None, None], wx.astype(ft)[None, :, None]
    one = ft(1.0)
    top = (one - wx) * f[y0][:, x0] + wx * f[y0][:, x1]
    bot = (one - wx) * f[y1][:, x0] + wx * f[y1][:, x1]
    return _rint_u8((one - wy) * top + wy * bot)


def grid_mask(mask, gys, gxs):
    H, W = mask.shape
    my = np.rint(np.clip(gys.astype(np.float32), 0, H - 1)).astype(np.int64)
    mx = np.rint(np.clip(gxs.astype(np.float32), 0, W - 1)).astype(np.int64)
    return mask[my][:, mx]


def grey_mean(img):
    """rint(mean grey), grey = (299 R + 587 G + 114 B) / 1000 -- in integers."""
    v = img.astype(np.int64)
    s = (299 * v[..., 0] + 587 * v[..., 1] + 114 * v[..., 2]).sum() if img.shape[2] == 3 else 1000 * v.sum()
    return float(np.rint(s / (1000.0 * img.shape[0] * img.shape[1])))


def hue(img, h, ft):
    v = img.astype(ft)
    R, G, B = v[..., 0], v[..., 1], v[..., 2]
    mx, mn = v.max(-1), v.min(-1)
    d = mx - mn
    with np.errstate(divide="ignore", invalid="ignore"):
        S = np.where(mx > 0, d / mx, ft(0))
        hr = (G - B) / d
        hr = np.where(hr < 0, hr + ft(6), hr)
        hg = (B - R) / d + ft(2)
        hb = (R - G) / d + ft(4)
    H = np.where(mx == R, hr, np.where(mx == G, hg, hb))
    H = np.where(d > 0, H / ft(6), ft(0)).astype(ft)
    H = H + ft(h)
    H = H - np.floor(H)
    H6 = H * ft(6)
    fi = np.floor(H6)
    f = H6 - fi
    i = fi.astype(np.int64) % 6
    one = ft(1)
    p, q, t = mx * (one - S), mx * (one - f * S), mx * (one - (one - f) * S)
    r = np.choose(i, [mx, q, p, p, t, mx])
    g = np.choose(i, [t, mx, mx, q, p, p])
    b = np.choose(i, [p, p, t, mx, mx, q])
    return np.clip(np.rint(np.stack([r, g, b], -1)), 0, 255).astype(np.uint8)


def run_view(img, mask, row, gys, gxs, noise, drop_u, Ho, Wo, mean, std, ft=np.float64):
    """img uint8 [Hs,Ws,Cs]; mask uint8 [Hs,Ws] or None; row: one ROW_DTYPE element; gys [Ho] / gxs [Wo] or None; noise float32
    [Cs,Ho,Wo] (scaled by sigma); drop_u float32 [Ho,Wo].  Returns (x [Cs,Ho,Wo] float32, y [Ho,Wo] int64 or None, m or -1)."""
    Cs = img.shape[2]
    x = resize_nearest(img, Ho, Wo)
    m = resize_nearest(mask, Ho, Wo) if mask is not None else None
    if row["hflip"]:
        x = x[:, ::-1]; m = m[:, ::-1] if m is not None else None
    if row["vflip"]:
        x = x[::-1]; m = m[::-1] if m is not None else None
    x = np.rot90(x, int(row["rot_k"])); m = np.rot90(m, int(row["rot_k"])) if m is not None else None
    cmean = -1.0
    for op, a, b in zip(row["op"], row["a"], row["b"]):
        a, b = ft(a), ft(b)
        if op == _lib.AUG_END:
            break
        if op == _lib.AUG_BC:
            x = _trunc_u8(x.astype(ft) * a + b * ft(255))
        elif op == _lib.AUG_NOISE:
            x = _trunc_u8(x.astype(ft) + np.transpose(noise, (1, 2, 0)).astype(ft))
        elif op == _lib.AUG_BLUR:
            x = box_blur(x, int(a))
        elif op == _lib.AUG_BRIGHT:
            x = _trunc_u8(x.astype(ft) * a)
        elif op == _lib.AUG_CONTRAST:
            cmean = grey_mean(x)
            x = _trunc_u8(x.astype(ft) * a + ft(cmean) * (ft(1) - a))
        elif op == _lib.AUG_SATURATE:
            if Cs == 3:
                v = x.astype(ft)
                grey = (ft(0.299) * v[..., 0] + ft(0.587) * v[..., 1] + ft(0.114) * v[..., 2])[..., None]
                x = np.rint(np.clip(grey + a * (v - grey), 0, 255)).astype(np.uint8)
        elif op == _lib.AUG_HUE:
            if Cs == 3:
                x = hue(x, a, ft)
        elif op == _lib.AUG_PIXDROP:
            x = np.where((drop_u < np.float32(a))[..., None], np.uint8(0), x)
        elif op == _lib.AUG_GRID:
            x = grid_sample(x, gys, gxs, ft)
            m = grid_mask(m, gys, gxs) if m is not None else None
        else:
            raise ValueError(op)
    t = x.astype(np.float32) / np.float32(255.0)
    t = (t - np.asarray(mean[:Cs], np.float32)) / np.asarray(std[:Cs], np.float32)
    return (np.ascontiguousarray(np.transpose(t, (2, 0, 1))), np.ascontiguousarray(m).astype(np.int64) if m is not None else None, cmean)


def grey_levels(x, mean, std):
    """Normalised [.., Cs, H, W] float32 -> the integer grey levels it was made from."""
    Cs = x.shape[-3]
    s = np.asarray(std[:Cs], np.float64).reshape(Cs, 1, 1)
    mu = np.asarray(mean[:Cs], np.float64).reshape(Cs, 1, 1)
    return np.rint((x.astype(np.float64) * s + mu) * 255.0).astype(np.int64)


def neu_rows(p):
    """AugParams of uaps_amd.augment -> the same draws as programs."""
    rows = P.empty_rows(len(p.ints))
    for b, (i, f) in enumerate(zip(p.ints, p.floats)):
        rows[b]["hflip"], rows[b]["vflip"], rows[b]["rot_k"] = i[0], i[1], i[2]
        ops = [("bc", f[0], f[1])]
        if i[3]:
            ops.append(("blur", int(i[3])))
        if i[4]:
            ops.append(("noise", f[2]))
        P.set_program(rows[b], ops)
    return rows


# ---- the cases of tests/test_gpu_augment_views.py::test_every_op_and_segment ---------------------------------------------------------
SHAPES = [((37, 53, 3), (32, 32)), ((40, 24, 1), (32, 32)), ((50, 30, 3), (64, 32)), ((32, 32, 3), (32, 32))]
SEEDS = [11, 12, 13, 14]                      # one per shape; see test_pipelines_host.py::test_case_seeds_keep_float32_ties_rare
DRAWN = ["ucc_strong", "dagm_labelled", "ucc_labelled", "ucc_strong"]      # the recipe of row 5
CAP = 1e-3                                    # share of an image's values that may differ from the float64 restatement (by one level)
MEAN, STD = P.IMAGENET_MEAN, P.IMAGENET_STD
B = 6


def case(i):
    """Inputs of shape i: B = 6 sources, rows 0-4 hand-set so that every opcode, every blur size, all four quarter turns, grid on
    and off, each of the three segments, and a CONTRAST behind BRIGHT and behind BLUR occur; row 5 is drawn from a recipe."""
    (Hs, Ws, Cs), (Ho, Wo) = SHAPES[i]
    rng = np.random.default_rng(SEEDS[i])
    img = rng.integers(0, 256, (B, Hs, Ws, Cs), dtype=np.uint8)
    mask = rng.integers(0, 4, (B, Hs, Ws), dtype=np.uint8)
    d = P.draw(DRAWN[i], B, rng, (Ho, Wo))
    rows = d.rows
    gys = np.tile(np.arange(Ho, dtype=np.float32), (B, 1)) if d.grid_ys is None else d.grid_ys
    gxs = np.tile(np.arange(Wo, dtype=np.float32), (B, 1)) if d.grid_xs is None else d.grid_xs
    sq = Ho == Wo
    # factors with no short decimal form: v * 0.9 sits ON an integer for every tenth grey level, where float32 and float64 truncate
    # differently; such inputs would measure the number format, not the kernel
    hand = [
        (1, 1, 1 if sq else 2, [("bc", 1.4371, 0.2113), ("grid",), ("noise", 7.0), ("blur", 7), ("contrast", 1.1537)]),
        (0, 0, 3 if sq else 0, [("blur", 3), ("bright", 0.9137), ("contrast", 0.8519), ("saturate", 1.2043), ("hue", 0.1311),
                                ("pixdrop", 0.05), ("noise", 4.0)]),
        (1, 0, 2, [("noise", 5.0), ("bc", 1.2113, 0.1037), ("blur", 5)]),
        (0, 1, 0, [("hue", -0.1713), ("saturate", 0.8117), ("bright", 1.1873), ("contrast", 1.0931), ("grid",), ("pixdrop", 0.1)]),
        (0, 0, 0, []),
    ]
    for b, (hf, vf, rot, ops) in enumerate(hand):
        rows[b]["hflip"], rows[b]["vflip"], rows[b]["rot_k"] = hf, vf, rot
        P.set_program(rows[b], ops)
        if rows[b]["grid_on"]:
            gys[b] = P.grid_map(Ho, 1.0 + rng.uniform(-0.3, 0.3, 5))
            gxs[b] = P.grid_map(Wo, 1.0 + rng.uniform(-0.3, 0.3, 5))
    sigma = np.zeros(B, np.float32)
    for b in range(B):
        for o, a in zip(rows[b]["op"], rows[b]["a"]):
            if o == _lib.AUG_NOISE:
                sigma[b] = a
    noise = (rng.standard_normal((B, Cs, Ho, Wo)).astype(np.float32) * sigma[:, None, None, None]).astype(np.float32)
    drop_u = rng.random((B, Ho, Wo), dtype=np.float32)
    return dict(img=img, mask=mask, draws=P.ViewDraws(rows, gys, gxs), noise=noise, drop_u=drop_u, out_size=(Ho, Wo))


def reference(c, ft=np.float64):
    Ho, Wo = c["out_size"]
    d = c["draws"]
    return [run_view(c["img"][b], c["mask"][b], d.rows[b], d.grid_ys[b], d.grid_xs[b], c["noise"][b], c["drop_u"][b], Ho, Wo,
                     MEAN, STD, ft) for b in range(B)]


def compare(x, ref_x):
    """(share of values that differ, largest difference in grey levels) between two normalised images."""
    a, b = grey_levels(x, MEAN, STD), grey_levels(ref_x, MEAN, STD)
    diff = np.abs(a - b)
    return float((diff > 0).mean()), int(diff.max())
