"""The reference of the instance tests (tests/test_instances_host.py, tests/test_gpu_instances.py): scipy.ndimage.label per class,
merged by first pixel; np.rint fixed-point sums; a numpy mask2rle / decode.  Every comparison built on it is exact."""
import functools

import numpy as np
import torch
from scipy import ndimage

DEV = torch.device("cuda:0")
S4 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
S8 = np.ones((3, 3), dtype=int)
TILE = 16                     # csrc/instances.hip labels 16 x 16 tiles in LDS (kTW, kTH) and merges them along their seams


def fixed_point(v):
    """q(v) = (int64) rint(clamp(v, -65536, 65536) * 2^24) in fp32, NaN -> 0."""
    v = np.asarray(v, dtype=np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    v = np.minimum(np.maximum(v, np.float32(-65536)), np.float32(65536)).astype(np.float32)
    return np.rint(v * np.float32(16777216.0)).astype(np.int64)


def label_image(m, maps, connectivity, background, min_area, max_instances):
    """One image [H,W]: (labels int32 [H,W], count, table int64 [max_instances,9])."""
    H, W = m.shape
    gid = np.zeros((H, W), dtype=np.int64)          # scipy's labels of every class, made distinct
    n_all = 0
    for c in np.unique(m):
        if background is not None and c == background:
            continue
        lab, n = ndimage.label(m == c, structure=S8 if connectivity == 8 else S4)
        gid += np.where(lab > 0, lab + n_all, 0)
        n_all += n
    flat = gid.reshape(-1)
    ids, first, area = np.unique(flat, return_index=True, return_counts=True)
    keep = (ids > 0) & (area >= min_area)
    ids, first, area = ids[keep], first[keep], area[keep]
    order = np.argsort(first)                       # merged by first pixel
    ids, first, area = ids[order], first[order], area[order]
    number = np.zeros(n_all + 1, dtype=np.int64)
    number[ids] = np.arange(1, len(ids) + 1)
    labels = number[gid]
    table = np.zeros((max_instances, 9), dtype=np.int64)
    n = min(len(ids), max_instances)
    table[:n, 0] = m.reshape(-1)[first[:n]]
    table[:n, 1] = area[:n]
    table[:n, 6] = first[:n]
    for k, sl in enumerate(ndimage.find_objects(labels, max_label=n)):
        table[k, 2:6] = (sl[0].start, sl[1].start, sl[0].stop, sl[1].stop)
    sel = (labels > 0) & (labels <= max_instances)
    for j, v in enumerate(maps):
        np.add.at(table[:, 7 + j], labels[sel] - 1, fixed_point(v)[sel])
    return labels.astype(np.int32), len(ids), table


def label_batch(mask, maps=(), connectivity=8, background=0, min_area=1, max_instances=256):
    """mask int64 [B,H,W] array, maps float32 [B,H,W] arrays -> (labels [B,H,W] int32, count [B] int32, table [B,M,9] int64)."""
    out = [label_image(mask[b], [v[b] for v in maps], connectivity, background, min_area, max_instances) for b in range(mask.shape[0])]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32), np.stack([o[2] for o in out]))


def assert_equal(res, ref, what=""):
    labels, count, table = ref
    got_t = res.table.cpu().numpy()
    assert np.array_equal(res.count.cpu().numpy(), count), (what, res.count.cpu().numpy(), count)
    assert res.labels.dtype == torch.int32 and np.array_equal(res.labels.cpu().numpy(), labels), what
    assert res.table.dtype == torch.int64 and got_t.shape == table.shape
    bad = np.argwhere(got_t != table)
    assert len(bad) == 0, (what, bad[:5], got_t[tuple(bad[0][:2])], table[tuple(bad[0][:2])])


def noise(B, H, W, density, C=4, seed=0):
    """Class noise: a pixel is foreground with probability `density`, its class uniform in 1..C-1."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((B, H, W)) < density, rng.integers(1, C, (B, H, W)), 0).astype(np.int64)


def random_maps(B, H, W, seed=1):
    rng = np.random.default_rng(seed)
    return [rng.random((B, H, W), dtype=np.float32), (rng.standard_normal((B, H, W)) * 3).astype(np.float32)]


def checkerboard(H, W, cls=1):
    y, x = np.mgrid[0:H, 0:W]
    return (((y + x) % 2 == 0) * cls).astype(np.int64)[None]


def spiral(H, W, cls=1):
    """A one-pixel-wide rectangular spiral with one-pixel gaps, from the outside in: one long chain, ONE component."""
    m = np.zeros((H, W), dtype=np.int64)
    y, x, dy, dx, turns = 0, 0, 0, 1, 0
    m[0, 0] = cls
    while turns < 2:
        ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        free = 0 <= ny < H and 0 <= nx < W and m[ny, nx] == 0 and not (0 <= fy < H and 0 <= fx < W and m[fy, fx] != 0)
        if free:
            y, x, turns = ny, nx, 0
            m[y, x] = cls
        else:
            dy, dx, turns = dx, -dy, turns + 1          # turn right
    return m[None]


def comb(H, W, cls=2):
    """A serpentine: full rows on every other line, joined alternately at the right and the left end -- one long chain."""
    m = np.zeros((H, W), dtype=np.int64)
    m[0::2] = cls
    for i, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if i % 2 == 0 else 0] = cls
    return m[None]


def diagonal(H, W, cls=3):
    m = np.zeros((H, W), dtype=np.int64)
    n = min(H, W)
    m[np.arange(n), np.arange(n)] = cls
    return m[None]


def corners(H, W, tile=TILE):
    """2 x 2 blocks centred on every four-tile corner (one pixel in each tile), alternating classes: under 8-connectivity one
    component per corner whose first pixel is the last pixel of the upper-left tile; plus single diagonal pairs across corners."""
    m = np.zeros((H, W), dtype=np.int64)
    k = 0
    for y in range(tile, H, tile):
        for x in range(tile, W, tile):
            if k % 2 == 0:
                m[y - 1:y + 1, x - 1:x + 1] = 1 + k % 3
            else:                                  # only the anti-diagonal pair: joined under 8-connectivity alone
                m[y - 1, x] = m[y, x - 1] = 1 + k % 3
            k += 1
    return m[None]


# ------------------------------------------------------------------------------------------------ run-length masks
def mask2rle_pairs(plane):
    """The runs of a binary plane over its column-major walk, 1-based starts: int64 [n,2] of (start, length)."""
    walk = np.zeros(plane.size + 2, dtype=np.int8)
    walk[1:-1] = np.asarray(plane, dtype=bool).reshape(-1, order="F")
    step = np.diff(walk)
    starts, ends = np.flatnonzero(step == 1), np.flatnonzero(step == -1)
    return np.stack([starts + 1, ends - starts], axis=1).astype(np.int64)


def rle_string(plane):
    return " ".join(str(v) for v in mask2rle_pairs(plane).reshape(-1))


def decode(pairs, H, W):
    flat = np.zeros(H * W, dtype=np.uint8)
    for s, n in pairs:
        flat[s - 1:s - 1 + n] = 1
    return flat.reshape(H, W, order="F")


def encode_batch(mask, classes):
    """mask [B,H,W], any int64 class values -> (col_offsets int32 [B * n * W + 1], pairs int32 [total,2]) in the layout of
    uaps_rle_count / uaps_rle_encode: segment j = b * n + c; a run belongs to the column its start lies in."""
    B, H, W = mask.shape
    per_col, pairs = [], []
    for b in range(B):
        for c in classes:
            p = mask2rle_pairs(mask[b] == c)
            pairs.append(p)
            per_col.append(np.bincount((p[:, 0] - 1) // H, minlength=W))
    per_col = np.concatenate(per_col)
    col_offsets = np.concatenate([[0], np.cumsum(per_col)]).astype(np.int32)
    return col_offsets, np.concatenate(pairs).astype(np.int32).reshape(-1, 2)


def decode_batch(pairs, offsets, B, H, W, classes, dtype=np.int64):
    """The plane-restricted decode of segments j = b * n + c, classes in order (later classes win): [B,H,W] of `dtype`.  Runs may be
    unordered, overlap, and leave the plane on either side; what leaves it is dropped."""
    out = np.zeros((B, H * W), dtype=dtype)
    for b in range(B):
        for k, c in enumerate(classes):
            j = b * len(classes) + k
            for s, n in pairs[offsets[j]:offsets[j + 1]]:
                lo, hi = max(int(s) - 1, 0), min(int(s) - 1 + int(n), H * W)
                if lo < hi:
                    out[b, lo:hi] = c
    return np.stack([f.reshape(H, W, order="F") for f in out])


@functools.lru_cache(maxsize=None)
def class_mask(B, H, W, C=3, seed=3):
    """Blobby label array with classes 0..C: long vertical and horizontal runs, runs through the column ends."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, C + 1, (B, (H + 3) // 4, (W + 2) // 3)).repeat(4, axis=1).repeat(3, axis=2)[:, :H, :W]
    return np.ascontiguousarray(m).astype(np.int64)
