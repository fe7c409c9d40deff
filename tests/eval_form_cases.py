"""The kernel forms of the evaluation chain, one small record per case (tests/test_eval_form_table.py, tests/test_gpu_eval_forms.py):
csrc/instances.hip (uaps_label_instances, uaps_rle_count / _encode / _decode), csrc/surface.hip (uaps_edt_sq,
uaps_surface_distances) and csrc/match.hip (uaps_match_instances).

A case names the entry point, the shape, the element offset of every tensor view, the pattern and its seed, the call's arguments and
the form it is there to reach.  inputs(case) builds the host arrays, reference(case) the expected outputs with the references the
suite already has (instances_ref on scipy, surface_ref on scipy, match_ref by brute force); compare() is the one comparison of the GPU
test: every quantity is an integer and must be equal, there is no tolerance anywhere.

The dispatch facts the cases rely on are restated here in plain Python, so that the CPU test can show from the table and the
references alone that every form is reached:
  labelling   16 x 16 tiles; 256-pixel chunks, scanned per image in rounds of 1024 chunk words (4 words a lane); flatten and final walk
              1024 consecutive pixels a wave (16 groups of 64) and carry whole groups of one component
  run lengths B * n_classes * W words scanned by one workgroup in rounds of 1024
  columns     nseg = clamp(ceil(H / 16), 1, 16) row segments of S = ceil(H / nseg) rows, strips of 64 columns
  selection   three digit passes of 9 + 8 + 8 bits (bits 16-24, 8-15, 0-7 of a squared distance)
  matching    V = 4 pixels a lane when H * W % 4 == 0 and both label pointers are 16-byte aligned, else V = 1; a wave walks
              64 * V * 4 pixels"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import instances_ref as I
import match_ref as M
import surface_ref as S

TILE, CHUNK, SCAN_ROUND, LABEL_SPAN = 16, 256, 1024, 1024
MAX_SEG, SEG_ROWS, STRIP = 16, 16, 64
SEL_BITS = (9, 8, 8)
U8, I32, I64 = 1, 4, 8                        # UAPS_LABEL_*
NP_OF = {U8: np.uint8, I32: np.int32, I64: np.int64}
WIDE = (-5, 0, 1, 2 ** 32 + 1, 2 ** 40)       # class values that need all 64 bits: 1 and 2^32 + 1 agree modulo 2^32
FRACS = (0.0, 50.0, 95.0, 100.0)              # percentiles; the call takes percentile / 100.0


def chunks(H, W):
    return -(-(H * W) // CHUNK)


def scan_rounds(n):
    return -(-n // SCAN_ROUND)


def segments(H):
    nseg = min(max(-(-H // SEG_ROWS), 1), MAX_SEG)
    return nseg, -(-H // nseg)


def match_v(HW, off_pred, off_target):
    """Element offsets of the int32 views from a 16-byte aligned base."""
    return 4 if HW % 4 == 0 and off_pred % 4 == 0 and off_target % 4 == 0 else 1


def match_span(V):
    return 64 * V * 4


def first_differing_pass(a, b):
    """The digit pass in which two squared distances part: 0, 1, 2, or None when they are equal."""
    x, shift = int(a) ^ int(b), sum(SEL_BITS)
    for p, bits in enumerate(SEL_BITS):
        shift -= bits
        if x >> shift:
            return p
    return None


@dataclass(frozen=True)
class Case:
    id: str
    entry: str                  # "label", "rle", "decode", "edt", "surface", "match"
    shape: tuple                # (B, H, W)
    pattern: str
    seed: int = 0
    offs: tuple = ()            # ((tensor, elements the view is moved by), ...); 0 where not named
    args: tuple = ()            # ((argument, value), ...)
    forms: tuple = ()           # the forms the case is there to reach

    def off(self, name):
        return dict(self.offs).get(name, 0)

    def arg(self, name, default=None):
        return dict(self.args).get(name, default)


def _case(cid, entry, shape, pattern, seed=0, offs=None, forms=(), **args):
    return Case(cid, entry, tuple(shape), pattern, seed, tuple(sorted((offs or {}).items())), tuple(sorted(args.items(), key=lambda kv: kv[0])),
                tuple(forms))


# ------------------------------------------------------------------------------------------------ labelling
ODD = dict(mask=1, labels=1, count=3, table=1, map0=1, map1=3)     # int32 views at odd offsets; int64 views 8-byte aligned only
SPARSE_PLANTS = ((511, 10, 3), (512, 300, 4), (0, 40, 3), (200, 100, 5))       # (row, first column, length) of runs in cleared ground


def seam_links(H, W):
    """Isolated pairs of pixels, each joined through ONE neighbour relation across a tile seam: up-right, up-left and up across every
    row seam, down-left, up-left and left across every column seam.  The diagonal ones are components under 8-connectivity alone."""
    m = np.zeros((H, W), dtype=np.int64)
    for y in range(TILE, H, TILE):
        for x, dx in ((3, 1), (8, -1), (12, 0)):
            if x + 1 < W:
                m[y, x] = m[y - 1, x + dx] = 1
    for x in range(TILE, W, TILE):
        for y, dy in ((3, 1), (8, -1), (12, 0)):
            if y + 1 < H:
                m[y, x] = m[y + dy, x - 1] = 2
    return m


def label_mask(c):
    B, H, W = c.shape
    p = c.pattern
    if p == "sparse":                           # sparse noise and a few planted runs, two of them in the chunks from 1024 on
        m = I.noise(B, H, W, 0.06, 4, seed=c.seed)
        for k, (y, x, n) in enumerate(SPARSE_PLANTS):
            m[:, max(y - 1, 0):y + 2, x - 2:x + n + 2] = 0
            m[:, y, x:x + n] = 1 + k % 3
        return m
    if p == "full":
        return np.full(c.shape, 2, dtype=np.int64)
    if p == "rows2":
        m = np.full(c.shape, 1, dtype=np.int64)
        m[:, 1::2] = 3
        return m
    if p == "full_empty_full":
        m = np.full(c.shape, 2, dtype=np.int64)
        m[1] = 0
        return m
    if p in ("spiral", "comb", "diagonal", "corners", "links"):
        m = I.noise(B, H, W, 0.4, 4, seed=c.seed)
        m[0] = seam_links(H, W) if p == "links" else getattr(I, p)(H, W)[0]
        return m
    if p == "wide":                             # 3 x 4 blocks of the five wide values; 1 and 2^32 + 1 side by side in the corner
        rng = np.random.default_rng(c.seed)
        m = np.array(WIDE, dtype=np.int64)[rng.integers(0, 5, (B, -(-H // 3), -(-W // 4)))].repeat(3, axis=1).repeat(4, axis=2)[:, :H, :W]
        m = np.ascontiguousarray(m)
        m[:, 0:2, 0:3], m[:, 0:2, 3:6] = 1, 2 ** 32 + 1
        return m
    if p == "noise":
        return I.noise(B, H, W, c.arg("density", 0.4), 4, seed=c.seed)
    if p == "bands":                            # noise and, per image, a solid band across a 1024-pixel wave boundary of the batch
        m = I.noise(B, H, W, 0.15, 4, seed=c.seed)
        for b in range(B):
            edge = -(-(b * H * W + 1) // LABEL_SPAN) * LABEL_SPAN - b * H * W          # the first boundary inside image b
            y = edge // W
            m[b, y - 2:y + 3, :] = 1 + b % 3
        return m
    raise ValueError(p)


def label_maps(c):
    B, H, W = c.shape
    maps = I.random_maps(B, H, W, seed=c.seed + 1)[:c.arg("n_maps", 0)]
    if c.arg("special") and maps:               # inside the bands: the clamp rule and NaN -> 0
        for b in range(B):
            y = (-(-(b * H * W + 1) // LABEL_SPAN) * LABEL_SPAN - b * H * W) // W
            maps[0][b, y, 0::7], maps[0][b, y, 1::7], maps[0][b, y + 1, 2::5] = np.nan, 1e9, -np.inf
            maps[0][b, y - 1, 3::6], maps[0][b, y - 1, 4::6] = np.inf, -1e9
            if len(maps) > 1:
                maps[1][b, y, 3::7], maps[1][b, y - 1, 0::4], maps[1][b, y + 1, 1::6] = -1e9, np.inf, np.nan
    return maps


def label_inputs(c):
    d = dict(mask=label_mask(c))
    for k, v in enumerate(label_maps(c)):
        d[f"map{k}"] = v
    return d


def label_reference(c, inp):
    maps = [inp[k] for k in ("map0", "map1") if k in inp]
    labels, count, table = I.label_batch(inp["mask"], maps, c.arg("connectivity", 8), c.arg("background", 0), c.arg("min_area", 1),
                                         c.arg("max_instances", 64))
    return dict(labels=labels, count=count, table=table)


def _label_cases():
    out = []
    for ma in (1, 3):
        out.append(_case(f"label-scan-min{ma}", "label", (2, 513, 513), "sparse", 5, ODD, ("scan-multi-round", "scan-partial-quad"),
                         min_area=ma, max_instances=16384))
    for shape in ((3, 9, 64), (3, 8, 72)):
        for p in ("full", "rows2", "full_empty_full"):
            out.append(_case(f"label-carry-{shape[1]}x{shape[2]}-{p}", "label", shape, p, 0, ODD, ("carry-image-boundary",), n_maps=2,
                             max_instances=16))
    for shape in ((2, 17, 31), (2, 33, 16), (1, 16, 17), (1, 31, 18), (1, 17, 33)):   # the last: two four-tile corners
        for p in ("spiral", "comb", "diagonal", "corners", "links"):
            for conn in (4, 8):
                out.append(_case(f"label-seam-{shape[1]}x{shape[2]}-{p}-c{conn}", "label", shape, p, 3 * shape[1] + shape[2], ODD,
                                 ("seam-ragged",), connectivity=conn, max_instances=512, n_maps=1))
    for name, bg in (("m5", -5), ("big", 2 ** 32 + 1), ("absent", 7), ("none", None)):
        out.append(_case(f"label-wide-bg-{name}", "label", (2, 19, 21), "wide", 11, ODD, ("int64-classes",), background=bg, max_instances=128,
                         connectivity=4))
    for mi in (1, 7):
        out.append(_case(f"label-overflow-{mi}", "label", (2, 21, 70), "noise", 7, ODD, ("overflow-maps",), max_instances=mi, n_maps=2))
    for nm in (1, 2):
        out.append(_case(f"label-maps-{nm}", "label", (2, 30, 50), "bands", 9, ODD, ("maps-unaligned",), n_maps=nm, special=True,
                         max_instances=512))
    out.append(_case("label-aligned", "label", (2, 21, 70), "noise", 7, None, ("aligned",), max_instances=512, n_maps=2, min_area=2))
    return out


# ------------------------------------------------------------------------------------------------ run-length masks
def rle_mask(c):
    """Blocks of the call's classes and of one value that is none of them."""
    B, H, W = c.shape
    classes = c.arg("classes")
    if c.pattern == "crossing":                 # one run through every column edge of every plane
        return np.full(c.shape, classes[0], dtype=np.int64)
    rng = np.random.default_rng(c.seed)
    vals = np.array(tuple(classes) + (c.arg("other", 77),), dtype=np.int64)
    m = np.ascontiguousarray(vals[rng.integers(0, len(vals), (B, -(-H // 2), -(-W // 3)))].repeat(2, axis=1).repeat(3, axis=2)[:, :H, :W])
    if W > 1:                                   # a run starts in the very last word of the scan: the last column of the last segment
        m[B - 1, 0, W - 1], m[B - 1, H - 1, W - 2] = classes[-1], vals[-1]
    return m


def rle_reference(c, inp):
    col_offsets, pairs = I.encode_batch(inp["mask"], c.arg("classes"))
    return dict(col_offsets=col_offsets, pairs=pairs)


def decode_inputs(c):
    B, H, W = c.shape
    classes, p = c.arg("classes"), c.pattern
    if p == "roundtrip":                        # the runs of a block mask, as uaps_rle_encode leaves them
        mask = rle_mask(c)
        col_offsets, pairs = I.encode_batch(mask, classes)
        return dict(pairs=pairs, offsets=np.ascontiguousarray(col_offsets[::W]))
    segs = {"none": [[] for _ in range(B * len(classes))],
            # unordered, overlapping inside a class and between the two classes
            "overlap": [[(7, 4), (1, 3), (2, 5)], [(3, 2), (9, 4)], [], [(12, 1), (1, 12)]],
            # empty segments in front of, between and behind the others
            "empty_segments": [[], [], [(2, 3)], [], [], [(1, 1), (5, 2)], [(4, 4)], [], []],
            # (2, 3, 5): starts at and below 0, ends up to 4 positions past H * W = 15
            "clip": [[(0, 3), (14, 5)], [(-3, 5), (16, 3)], [(-2, 2), (13, 6)], [(1, 19), (0, 1)]]}[p]
    assert len(segs) == B * len(classes)
    flat = [r for s in segs for r in s]
    return dict(pairs=np.array(flat, dtype=np.int32).reshape(-1, 2), offsets=np.cumsum([0] + [len(s) for s in segs]).astype(np.int32))


def decode_reference(c, inp):
    B, H, W = c.shape
    return dict(out=I.decode_batch(inp["pairs"], inp["offsets"], B, H, W, c.arg("classes"), np.uint8 if c.arg("uint8") else np.int64))


RLE_LENGTHS = {1023: ((1, 3, 341), 3), 1024: ((2, 1, 64), 8), 1025: ((5, 3, 41), 5), 2049: ((3, 1, 683), 1), 4100: ((5, 3, 205), 4)}
EIGHT = (3, -9, 2 ** 32 + 1, 1, 0, 250, 2 ** 40, 17)


def _rle_cases():
    out = []
    offs = dict(mask=1, col_offsets=1, pairs=3)
    for n, (shape, nc) in RLE_LENGTHS.items():
        out.append(_case(f"rle-scan-{n}", "rle", shape, "blocks", n, offs, (f"rle-scan-{n}",), classes=EIGHT[:nc]))
    out.append(_case("rle-w1", "rle", (3, 9, 1), "blocks", 2, offs, ("rle-W1",), classes=(1, -9)))
    out.append(_case("rle-crossing", "rle", (2, 3, 37), "crossing", 0, offs, ("rle-crossing",), classes=(2 ** 32 + 1, 1)))
    out.append(_case("rle-aligned", "rle", (2, 6, 70), "blocks", 4, None, ("aligned",), classes=(1, 2, 3)))
    for u8 in (0, 1):
        t = "u8" if u8 else "i64"
        cl = (5, 250, 9) if u8 else (5, 2 ** 32 + 1, -9)
        o = dict(pairs=1, offsets=1, out=1)
        out.append(_case(f"decode-roundtrip-{t}", "decode", (2, 7, 31), "roundtrip", 6, o, ("decode-odd-offsets",), classes=cl, uint8=u8))
        out.append(_case(f"decode-none-{t}", "decode", (2, 3, 5), "none", 0, o, ("decode-no-runs",), classes=cl[:2], uint8=u8))
        out.append(_case(f"decode-overlap-{t}", "decode", (2, 3, 4), "overlap", 0, o, ("decode-overlap",), classes=cl[:2], uint8=u8))
        out.append(_case(f"decode-empty-{t}", "decode", (3, 2, 4), "empty_segments", 0, o, ("decode-empty-segments",), classes=cl, uint8=u8))
        out.append(_case(f"decode-clip-{t}", "decode", (2, 3, 5), "clip", 0, o, ("decode-clip",), classes=cl[:2], uint8=u8))
    return out


# ------------------------------------------------------------------------------------------------ distance transform, surface distances
SEG_H, SEG_W = (16, 17, 32, 33, 240, 241, 256, 257), (2, 64, 65)
BLOB_SEEDS = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1, 8: 2}     # per C: a seed with at least half of the pairs valid (the table test)


def segment_maps(H, W):
    """(pred, target) [2,H,W]: class 1 lies in the first row segment of its columns only, class 2 in the last only, class 3 in
    both with nothing between; thin lines, so every pixel of theirs is a surface pixel.  Image 1 swaps the two sides."""
    p, t = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    for arr, dy in ((p, 0), (t, 2)):
        arr[1 + dy, 0::3] = 1
        arr[3 + dy, 1::3] = 3
        arr[H - 1, 0::3] = 2
        arr[H - 1, 1::3] = 3
    return np.stack([p, t]), np.stack([t, p])


def selection_maps(W=512):
    """One-row images of two classes: the target's one pixel of class 1 at column 0, the prediction's at column 1 and at a column that
    sets the third value: pooled (1, 1, d^2), d = 300, 17, 3: the two upper ranks part in pass 0, 1, 2.  Image 3: one pixel a side."""
    p, t = np.zeros((4, 1, W), dtype=np.int64), np.zeros((4, 1, W), dtype=np.int64)
    t[:, 0, 0] = 1
    for b, far in enumerate((300, 17, 3)):
        p[b, 0, 1] = p[b, 0, far] = 1
    p[3, 0, 5] = 1
    return p, t


def score_maps(c):
    """Scores from a handful of values, so that ties, -0.0 against +0.0 and infinities meet at many pixels."""
    B, H, W = c.shape
    rng = np.random.default_rng(c.seed)
    vals = np.array([-np.inf, -1.0, -0.0, 0.0, 0.5, np.inf], dtype=np.float32)
    return vals[rng.integers(0, len(vals), (B, c.arg("C"), H, W))]


def outside_labels(c, dtype, seed):
    """Labels 0 .. C-1 with a fifth of the pixels outside [0, C): above it, far above it, and negative where the type has a sign."""
    B, H, W = c.shape
    rng = np.random.default_rng(seed)
    m = rng.integers(0, c.arg("C"), c.shape).astype(np.int64)
    out = {U8: (5, 200, 255), I32: (5, -3, 2 ** 31 - 1, -2 ** 31), I64: (5, -3, 2 ** 32 + 1, 2 ** 40, -2 ** 63)}[dtype]
    hit = rng.random(c.shape) < 0.2
    return np.where(hit, np.array(out, dtype=np.int64)[rng.integers(0, len(out), c.shape)], m)


def surface_inputs(c):
    B, H, W = c.shape
    p = c.pattern
    dp, dt = c.arg("pred_dtype", I64), c.arg("target_dtype", I64)
    if p == "segments":
        pred, target = segment_maps(H, W)
    elif p == "selection":
        pred, target = selection_maps(W)
    elif p == "outside":
        pred, target = outside_labels(c, dp, c.seed), outside_labels(c, dt, c.seed + 1)
    elif p == "scores":
        scores = score_maps(c)
        return dict(scores=scores, pred=np.argmax(scores, axis=1).astype(np.int64), target=S.class_noise(B, H, W, c.arg("C"), c.seed)[1])
    else:
        pred, target = S.PATTERNS[p](B, H, W, c.arg("C"), c.seed)
    return dict(pred=pred, target=target)


def surface_reference(c, inp):
    tol = c.arg("tol_d2", 0) if c.arg("has_tolerance", 0) else None
    return dict(table=S.table(inp["pred"], inp["target"], c.arg("C"), c.arg("percentile", 95.0), None, tol))


EDT_VALUE = {U8: 255, I32: -7, I64: 2 ** 32}  # what "not a feature" is written as: any value but 0, the int64 one with 32 low zero bits


def edt_inputs(c):
    B, H, W = c.shape
    pred = segment_maps(H, W)[0][0]
    return dict(mask=np.stack([pred != k for k in (1, 2, 3)]))     # B = 3: the zero pixels are the class's


def edt_reference(c, inp):
    return dict(out=np.stack([S.edt_sq(m) for m in inp["mask"]]).astype(np.int32))


def _surface_cases():
    out = []
    offs = dict(pred=1, target=1, table=1, scores=1)
    for C in range(1, 9):
        out.append(_case(f"surf-blobs-C{C}", "surface", (2, 37, 53), "blobs", BLOB_SEEDS[C], offs, (f"col-C{C}",), C=C))
    for p in ("absent", "filled"):
        out.append(_case(f"surf-{p}", "surface", (2, 37, 53), p, 3, offs, ("invalid-pairs",), C=4))
    for H in SEG_H:
        for W in SEG_W:
            out.append(_case(f"surf-seg-{H}x{W}", "surface", (2, H, W), "segments", 0, offs, (f"col-nseg-{segments(H)[0]}",), C=4))
            for d in (U8, I32, I64):
                out.append(_case(f"edt-seg-{H}x{W}-d{d}", "edt", (3, H, W), "segments", 0, dict(mask=1, out=1), ("edt-dtype",), dtype=d))
    for q in FRACS:
        out.append(_case(f"surf-select-{q:g}", "surface", (4, 1, 512), "selection", 0, offs, ("selection",), C=2, percentile=q))
        out.append(_case(f"surf-blobs-q{q:g}", "surface", (2, 37, 53), "blobs", 1, offs, ("selection",), C=4, percentile=q))
    for has, tol in ((1, 0), (1, 1), (1, 2 ** 25), (0, 9)):
        out.append(_case(f"surf-tol-{has}-{tol}", "surface", (2, 37, 53), "blobs", 1, offs, ("tolerance",), C=4, has_tolerance=has, tol_d2=tol))
    for C in (1, 5):
        out.append(_case(f"surf-scores-C{C}", "surface", (2, 19, 23), "scores", 4, offs, ("scores",), C=C, scores=True))
    for dp in (U8, I32, I64):
        for dt in (U8, I32, I64):
            out.append(_case(f"surf-dtype-{dp}-{dt}", "surface", (2, 19, 23), "outside", 8, offs, ("dtype-pairs",), C=3, pred_dtype=dp,
                             target_dtype=dt))
    out.append(_case("surf-aligned", "surface", (2, 37, 53), "blobs", 2, None, ("aligned",), C=4, has_tolerance=1, tol_d2=4))
    return out


# ------------------------------------------------------------------------------------------------ matching
STRIDES = ((1, 1), (1, 65), (65, 1), (33, 64), (40, 129))
WIDE_CLASS = {1: -5, 2: 2 ** 32 + 1, 3: 1}    # table classes of the wide-class case: 2^32 + 1 and 1 must stay apart


def stripes(B, H, W, seed):
    """Vertical stripes against horizontal ones, classes 1 - 3: every prediction crosses every target, in w * h pixels, and the
    crossing counts where the two classes agree -- a dense pair matrix of many different words.  Stripes are 1 - 3 pixels wide, from
    the 33rd prediction and the 65th / 129th target on up to 5 / 7 (those three exactly that): largest intersections lie behind every 32-row round and 64-column
    group too.  Stripes 1, 65 and 129 of either side are of class 2, so that the one-row and one-column matrices hold a counted word."""
    rng = np.random.default_rng(seed)
    pred, gt = np.zeros((B, H, W), dtype=np.int64), np.zeros((B, H, W), dtype=np.int64)
    for b in range(B):
        x = k = 0
        while x < W:
            w = 5 if k == 32 else int(rng.integers(1, 4 + 2 * (k > 32)))
            pred[b, :, x:x + w] = 2 if k % 64 == 0 else rng.integers(1, 4)
            x, k = x + w + 1, k + 1
        y = k = 0
        while y < H:
            h = {64: 5, 128: 7}.get(k) or int(rng.integers(1, 4 + 2 * (k > 64) + 2 * (k > 128)))
            gt[b, y:y + h, :] = 2 if k % 64 == 0 else rng.integers(1, 4)
            y, k = y + h + 1, k + 1
    return pred, gt


def crafted(thr_images=True):
    """(6, 3, 12), class 1 in row 1: image 0 one prediction over two targets of four pixels each, image 1 the same the other way
    round; images 2 - 5: inter == thr * union exactly at 0.5 and 0.75, and each with one more pixel."""
    pred, gt = np.zeros((6, 3, 12), dtype=np.int64), np.zeros((6, 3, 12), dtype=np.int64)
    pred[0, 1, 0:9] = 1; gt[0, 1, 0:4] = 1; gt[0, 1, 5:9] = 1
    gt[1, 1, 0:9] = 1; pred[1, 1, 0:4] = 1; pred[1, 1, 5:9] = 1
    pred[2, 1, 0:3] = 1; gt[2, 1, 0:6] = 1                      # 3 of 6
    pred[3, 1, 0:4] = 1; gt[3, 1, 0:6] = 1                      # 4 of 6
    pred[4, 1, 0:3] = 1; gt[4, 1, 0:4] = 1                      # 3 of 4
    pred[5, 1, 0:4] = 1; gt[5, 1, 0:4] = 1                      # 4 of 4
    return pred, gt


@functools.lru_cache(maxsize=None)
def match_masks(pattern, shape, seed):
    B, H, W = shape
    if pattern == "stripes":
        return stripes(B, H, W, seed)
    if pattern == "crafted":
        return crafted()
    if pattern == "full":
        return np.full(shape, 2, dtype=np.int64), np.full(shape, 2, dtype=np.int64)
    gt = I.noise(B, H, W, {"noise": 0.7, "sparse": 0.1}[pattern], 4, seed=seed)
    return M.redraw(gt, 0.15, 4, seed=seed + 1), gt


@functools.lru_cache(maxsize=None)
def _labelled(pattern, shape, seed, conn, mp, mg):
    pred, gt = match_masks(pattern, shape, seed)
    return I.label_batch(pred, (), conn, 0, 1, mp), I.label_batch(gt, (), conn, 0, 1, mg)


def match_inputs(c):
    (lp, cp, tp), (lg, cg, tg) = _labelled(c.pattern, c.shape, c.seed, c.arg("connectivity", 8), c.arg("max_pred"), c.arg("max_gt"))
    lp, cp, tp, lg, cg, tg = (a.copy() for a in (lp, cp, tp, lg, cg, tg))
    if c.arg("odd_counts"):                     # per image: 0, negative, far above the table, the true one
        for cnt, vals in ((cp, (0, -3, 10 ** 6)), (cg, (-1, 10 ** 6, 0))):
            for b, v in enumerate(vals):
                cnt[b] = v
        for lab in (lp, lg):                    # and labels that are no component's: negative ones, and numbers above every table
            lab[:, 0, 0::3] = -1
            lab[:, 1, 1::4] = -(2 ** 31)
            lab[:, 2, 0::5] = 2 ** 31 - 1
    if c.arg("wide_classes"):
        for t in (tp, tg):
            col = t[..., 0]
            col[...] = np.select([col == k for k in WIDE_CLASS], list(WIDE_CLASS.values()), col)
    return dict(pred_labels=lp, target_labels=lg, pred_count=cp, target_count=cg, pred_table=tp, target_table=tg)


def match_reference(c, inp):
    pred, target, counts, _ = M.match_batch((inp["pred_labels"], inp["pred_count"], inp["pred_table"]),
                                            (inp["target_labels"], inp["target_count"], inp["target_table"]), c.arg("num_classes", 4),
                                            c.arg("thr", 0.5), bool(c.arg("agnostic", 0)))
    return dict(pred_out=pred, target_out=target, counts=counts)


FORMS_SHAPE = (3, 20, 36)                       # H * W = 720: three waves at V = 4, nine at V = 1


def _match_cases():
    out = []
    o = dict(pred_table=1, target_table=1, pred_out=1, target_out=1, counts=1, pred_count=1, target_count=3)
    kw = dict(max_pred=150, max_gt=170)
    for tag, po, to, shape, form in (("v4", 0, 0, FORMS_SHAPE, "pair-V4"), ("v1-pred", 1, 0, FORMS_SHAPE, "pair-V1-pred-off"),
                                     ("v1-target", 0, 2, FORMS_SHAPE, "pair-V1-target-off"), ("v1-hw", 0, 0, (3, 21, 35), "pair-V1-hw")):
        out.append(_case(f"match-{tag}", "match", shape, "noise", 21, dict(o, pred_labels=po, target_labels=to), (form,), **kw))
    out.append(_case("match-images-70x2x2", "match", (70, 2, 2), "noise", 22, o, ("many-images-per-wave",), max_pred=3, max_gt=5))
    out.append(_case("match-images-50x1x3", "match", (50, 1, 3), "noise", 23, o, ("many-images-per-wave",), max_pred=2, max_gt=3))
    out.append(_case("match-carry", "match", (3, 9, 64), "full", 0, o, ("carry-images",), max_pred=4, max_gt=6))
    for mp, mg in STRIDES:
        out.append(_case(f"match-strides-{mp}x{mg}", "match", (2, 500, 270), "stripes", 24, o, ("matrix-strides",), max_pred=mp, max_gt=mg,
                         connectivity=4))
    out.append(_case("match-counts", "match", (4, 20, 36), "noise", 25, o, ("odd-counts",), odd_counts=True, max_pred=40, max_gt=30))
    for thr in (0.5, 0.75):
        out.append(_case(f"match-crafted-{thr}", "match", (6, 3, 12), "crafted", 0, o, ("ties", "threshold-exact"), thr=thr, max_pred=3,
                         max_gt=2))
    for ag in (0, 1):
        out.append(_case(f"match-agnostic-{ag}", "match", FORMS_SHAPE, "noise", 21, o, ("agnostic",), agnostic=ag, thr=0.75, **kw))
    out.append(_case("match-nc1", "match", FORMS_SHAPE, "noise", 21, o, ("classes-outside", "nc-1"), num_classes=1, **kw))
    out.append(_case("match-nc64", "match", FORMS_SHAPE, "noise", 21, o, ("nc-64",), num_classes=64, **kw))
    out.append(_case("match-wide-classes", "match", FORMS_SHAPE, "noise", 21, o, ("classes-outside", "int64-classes"), wide_classes=True,
                     num_classes=4, **kw))
    return out


STALE = ("match-strides-40x129", "match-sparse", "match-strides-40x129")      # dense, sparse, dense on one workspace
SPARSE_CASE = _case("match-sparse", "match", (2, 500, 270), "sparse", 26, dict(pred_table=1, target_table=1), ("stale",), max_pred=24,
                    max_gt=40)

# ------------------------------------------------------------------------------------------------ the table
CASES = _label_cases() + _rle_cases() + _surface_cases() + _match_cases() + [SPARSE_CASE]
FORMS = (("scan-multi-round", "scan-partial-quad", "carry-image-boundary", "seam-ragged", "int64-classes", "overflow-maps", "maps-unaligned")
         + tuple(f"rle-scan-{n}" for n in RLE_LENGTHS) + ("rle-W1", "rle-crossing")
         + ("decode-odd-offsets", "decode-no-runs", "decode-overlap", "decode-empty-segments", "decode-clip")
         + tuple(f"col-C{C}" for C in range(1, 9)) + tuple(f"col-nseg-{n}" for n in (1, 2, 3, 15, 16))
         + ("invalid-pairs", "edt-dtype", "selection", "tolerance", "scores", "dtype-pairs")
         + ("pair-V4", "pair-V1-pred-off", "pair-V1-target-off", "pair-V1-hw", "many-images-per-wave", "carry-images", "matrix-strides",
            "odd-counts", "ties", "threshold-exact", "agnostic", "classes-outside", "nc-1", "nc-64", "stale", "aligned"))
BY_ID = {c.id: c for c in CASES}

_INPUTS = dict(label=label_inputs, rle=lambda c: dict(mask=rle_mask(c)), decode=decode_inputs, edt=edt_inputs, surface=surface_inputs,
               match=match_inputs)
_REFERENCE = dict(label=label_reference, rle=rle_reference, decode=decode_reference, edt=edt_reference, surface=surface_reference,
                  match=match_reference)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """name -> host array; computed once per case and shared: treat as read-only."""
    d = _INPUTS[c.entry](c)
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(c):
    """name -> the expected array of every output of the case; computed once and shared: treat as read-only."""
    d = _REFERENCE[c.entry](c, inputs(c))
    for a in d.values():
        a.setflags(write=False)
    return d


def ids(entry):
    return [c.id for c in CASES if c.entry == entry]


def compare(ref, got):
    """The comparison of the GPU test: every output of the reference, element for element.  -> the list of what differs."""
    bad = []
    for k, want in ref.items():
        g = got.get(k)
        if g is None:
            bad.append(f"{k}: missing")
        elif g.shape != want.shape:
            bad.append(f"{k}: shape {g.shape}, expected {want.shape}")
        elif g.dtype.kind not in "iu" or not np.array_equal(g.astype(np.int64), want.astype(np.int64)):
            at = np.argwhere(np.asarray(g != want))
            first = tuple(at[0]) if len(at) else ()
            bad.append(f"{k}: {len(at)} of {want.size} differ, first at {first}: {g[first] if len(at) else g.dtype} != {want[first] if len(at) else want.dtype}")
    return bad
