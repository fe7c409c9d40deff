"""The reference of the threshold-sweep tests (tests/test_curves_host.py, tests/test_gpu_curves.py): brute force -- one np.bincount per
(image, row, event), plain loops over regions and bins -- written from the contract in include/uaps_hip.h, independent of
uaps_amd/curves.py.  Probability inputs are binned by the fp32 rule; logits go through a float64 softmax (sigmoid) first, and the
generator keeps every scored value 2^-18 away from a bin edge so that the device's expf cannot move a pixel into another bin:
expf is within 2 ulp, at most 7 adds, one division and the bin multiply follow -- below 7.2e-7 absolute on a probability; 2^-18 =
3.8e-6 is four times that."""
import functools

import numpy as np

import instances_ref as R

DEV = R.DEV
SHAPES = ((1, 1, 1), (1, 1, 45), (3, 37, 53), (2, 7, 300), (2, 130, 70), (2, 256, 256))
ONE_LANE, FOUR_LANE = SHAPES[:3], SHAPES[3:]
CLASSES = (1, 2, 4, 8)
BINS = (2, 15, 1024, 4096)
PATTERNS = ("uniform", "saturated", "one_bin", "edges", "nans", "ignored")
MARGIN = 2.0 ** -18
F32 = np.float32


def bin_scalar(s, bins, lo=0.0, hi=1.0):
    """The bin of ONE score by the rule, step by step in fp32 scalars; None for a NaN."""
    s = F32(s)
    if np.isnan(s):
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        inv = F32(F32(bins) / F32(F32(hi) - F32(lo)))
        t = np.floor(F32(F32(s - F32(lo)) * inv))
    if t < 0:
        t = F32(0)
    if t > bins - 1:
        t = F32(bins - 1)
    return int(t)


def bins_of(s, bins, lo=0.0, hi=1.0):
    """The same over an array (no NaN in it)."""
    s = np.asarray(s, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        inv = F32(F32(bins) / F32(F32(hi) - F32(lo)))
        t = np.floor(((s - F32(lo)).astype(F32) * inv).astype(F32))
    return np.clip(t, 0, bins - 1).astype(np.int64)


def edge_values(bins_list=(15, 1024)):
    """Scores on and beside the edges: k / bins for every k, 1.0, the neighbours of edges, beyond both bounds, infinities, NaN, -0.0, a
    denormal."""
    v = []
    for bins in bins_list:
        e = (np.arange(bins + 1, dtype=np.float64) / bins).astype(F32)
        v += [e, np.nextafter(e, F32(-1)), np.nextafter(e, F32(2))]
    v.append(np.array([1.0, -0.0, 0.0, 1e-45, -1e-45, 1e-39, -1e-3, -7.0, 1.0000001, 1.5, 7.0, 3e38, -3e38, np.inf, -np.inf, np.nan, 0.5],
                      dtype=F32))
    return np.concatenate(v).astype(F32)


def softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def probabilities(S, from_logits):
    """[B,C,H,W] float32 scores as the rule bins them: the input, or the float64 softmax / sigmoid rounded to fp32 (the generator keeps
    them away from the edges, so the rounding cannot change a bin)."""
    if not from_logits:
        return np.asarray(S, dtype=F32)
    if S.shape[1] == 1:
        return (1.0 / (1.0 + np.exp(-S.astype(np.float64)))).astype(F32)
    return softmax64(S).astype(F32)


def rows_of(S, t, classes, top, from_logits):
    """[(score fp32 [B,H,W], event, counted, is NaN)] per row: the class rows, then the top row."""
    B, C, H, W = S.shape
    P = probabilities(S, from_logits)
    rows = []
    if C == 1:
        p, ok = P[:, 0], (t == 0) | (t == 1)
        for _ in classes:
            rows.append((p, t == 1, ok, np.isnan(p)))
        if top:
            pred = (S[:, 0] > 0) if from_logits else (p > F32(0.5))
            with np.errstate(invalid="ignore"):
                rows.append((np.maximum(p, (F32(1) - p).astype(F32)), pred == (t == 1), ok, np.isnan(p)))
        return rows
    ok = (t >= 0) & (t < C)
    for c in classes:
        rows.append((P[:, c], t == c, ok, np.isnan(P[:, c])))
    if top:
        bad = np.isnan(P).any(axis=1)
        am = np.zeros((B, H, W), dtype=np.int64)                  # arg-max of the INPUT, the lowest index among equal values
        best = S[:, 0].copy()
        with np.errstate(invalid="ignore"):
            for c in range(1, C):
                better = S[:, c] > best
                am[better] = c
                best[better] = S[:, c][better]
            score = P[:, 0].copy()
            for c in range(1, C):
                score = np.where(P[:, c] > score, P[:, c], score)
        rows.append((score, am == t, ok, bad))
    return rows


def histograms(rows, bins, lo, hi, want_sums):
    B, Rn = rows[0][0].shape[0], len(rows)
    hist = np.zeros((B, Rn, 2, bins), dtype=np.int64)
    qsum = np.zeros((B, Rn, 2, bins), dtype=np.int64) if want_sums else None
    nan = np.zeros((B, Rn), dtype=np.int64)
    for b in range(B):
        for r, (s, ev, ok, bad) in enumerate(rows):
            nan[b, r] = np.count_nonzero(ok[b] & bad[b])
            for e in (0, 1):
                sel = ok[b] & ~bad[b] & (ev[b] == bool(e))
                idx = bins_of(s[b][sel], bins, lo, hi)
                hist[b, r, e] = np.bincount(idx, minlength=bins)
                if want_sums:                                     # integers below 2^53 throughout: float64 weights add exactly
                    w = np.bincount(idx, weights=R.fixed_point(s[b][sel]).astype(np.float64), minlength=bins)
                    assert np.abs(w).max(initial=0.0) < 2.0 ** 52
                    qsum[b, r, e] = w.astype(np.int64)
    return hist, qsum, nan


def curves(S, t, classes=None, bins=1024, top=True, from_logits=False, regions=None, want_sums=False, lo=0.0, hi=1.0):
    """dict(hist, qsum, nan, pro_sum, n_regions, valid) of uaps_score_curves; regions = (labels, count, table) of label_batch.  A table
    row whose area is not positive is no region: it is not counted and adds nothing."""
    S, t = np.asarray(S, dtype=F32), np.asarray(t).astype(np.int64)
    B, C = S.shape[:2]
    classes = ([1] if C == 1 else list(range(1, C))) if classes is None else list(classes)
    hist, qsum, nan = histograms(rows_of(S, t, classes, top, from_logits), bins, lo, hi, want_sums)
    out = dict(hist=hist, qsum=qsum, nan=nan, pro_sum=None, n_regions=None, valid=np.ones(B, dtype=bool))
    if regions is None:
        return out
    labels, count, table = regions
    Mg = table.shape[1]
    P = probabilities(S, from_logits)
    pro = np.zeros((B, len(classes), bins), dtype=np.float64)
    n_reg = np.zeros((B, len(classes)), dtype=np.int64)
    for b in range(B):
        for r in range(min(int(count[b]), Mg)):
            c, area = int(table[b, r, 0]), int(table[b, r, 1])
            plane = 0 if (C == 1 and c == 1) else (c if (C > 1 and 0 <= c < C) else None)
            h = np.zeros(bins, dtype=np.int64)
            if plane is not None:
                s = P[b, plane][labels[b] == r + 1]
                h = np.bincount(bins_of(s[~np.isnan(s)], bins, lo, hi), minlength=bins)
            suffix = np.zeros(bins, dtype=np.int64)
            run = 0
            for i in range(bins - 1, -1, -1):
                run += int(h[i])
                suffix[i] = run
            for k, ck in enumerate(classes):
                if ck == c and area > 0:
                    n_reg[b, k] += 1
                    pro[b, k] += suffix.astype(np.float64) / np.float64(area)
    out.update(pro_sum=pro, n_regions=n_reg, valid=np.asarray(count) <= Mg)
    return out


def plane(score, pred, target, bins=1024, lo=0.0, hi=1.0, want_sums=False):
    score, pred, target = np.asarray(score, dtype=F32), np.asarray(pred).astype(np.int64), np.asarray(target).astype(np.int64)
    hist, qsum, nan = histograms([(score, pred == target, target >= 0, np.isnan(score))], bins, lo, hi, want_sums)
    return dict(hist=hist, qsum=qsum, nan=nan, pro_sum=None, n_regions=None, valid=np.ones(score.shape[0], dtype=bool))


def assert_result(res, ref, what="", pro_rel=0.0):
    """Every integer output exactly, and pro_sum bit for bit: both sides add IEEE double quotients in ascending region order."""
    for name in ("hist", "qsum", "nan", "n_regions"):
        got, want = getattr(res, name), ref[name]
        assert (got is None) == (want is None), (what, name)
        if want is not None:
            got = got.cpu().numpy()
            assert got.dtype == np.int64 and got.shape == want.shape, (what, name, got.shape, want.shape)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (what, name, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(res.valid.cpu().numpy(), ref["valid"]), what
    assert (res.pro_sum is None) == (ref["pro_sum"] is None), what
    if ref["pro_sum"] is not None:
        got, want = res.pro_sum.cpu().numpy(), ref["pro_sum"]
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.all(np.abs(got - want) <= pro_rel * np.abs(want)), (what, "pro_sum", np.abs(got - want).max())


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def targets(shape, C, ignored=False, seed=0):
    """int64 [B,H,W] blobs of classes 0 .. max(C, 2) - 1; ignored: a twentieth of the pixels carry -1, 255 or C."""
    B, H, W = shape
    rng = np.random.default_rng(seed + 31 * H + W)
    cell = 16 if min(H, W) >= 64 else 3
    t = rng.integers(0, max(C, 2), (B, H // cell + 1, W // cell + 1)).repeat(cell, axis=1).repeat(cell, axis=2)[:, :H, :W].astype(np.int64)
    if ignored:
        m = rng.random(shape)
        t = np.where(m < 0.02, -1, np.where(m < 0.04, 255, np.where(m < 0.05, max(C, 2), t)))
    t = np.ascontiguousarray(t)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def scores(pattern, shape, C, seed=0):
    """float32 [B,C,H,W] for the probability path."""
    B, H, W = shape
    rng = np.random.default_rng(seed + 7 * H + 13 * W + C)
    full = (B, C, H, W)
    if pattern in ("uniform", "ignored"):
        S = rng.random(full, dtype=F32)
    elif pattern == "saturated":
        S = (rng.random(full) < 0.5).astype(F32)
    elif pattern == "one_bin":
        S = np.full(full, 0.5, dtype=F32)
    elif pattern == "edges":
        e = edge_values()
        S = e[rng.integers(0, len(e), full)]
        S.reshape(-1)[:min(len(e), S.size)] = e[:S.size]
    elif pattern == "nans":
        S = rng.random(full, dtype=F32)
        S[rng.random(full) < 0.03] = np.nan
    else:
        raise KeyError(pattern)
    S = np.ascontiguousarray(S, dtype=F32)
    S.setflags(write=False)
    return S


def _near_edge(p, bins):
    """Is a float64 probability within MARGIN of an interior bin edge k / bins, 1 <= k <= bins - 1?"""
    k = np.clip(np.rint(p * bins), 1, bins - 1)
    return np.abs(p - k / bins) < MARGIN


@functools.lru_cache(maxsize=None)
def logits(shape, C, bins_list=BINS, seed=0, scale=3.0):
    """float32 [B,C,H,W] logits none of whose scored values -- every class probability, the maximum, and at C == 1 also 1 - p -- lies
    within MARGIN of a bin edge of any of `bins_list`: pixels that do are drawn again, at most 50 times."""
    B, H, W = shape
    rng = np.random.default_rng(seed + 5 * H + 3 * W + C)
    z = (rng.standard_normal((B, C, H, W)) * scale).astype(F32)
    for rounds in range(51):
        p = 1.0 / (1.0 + np.exp(-z.astype(np.float64))) if C == 1 else softmax64(z)
        vals = np.concatenate([p, 1.0 - p], axis=1) if C == 1 else p          # (the maximum is one of the class values)
        bad = np.zeros((B, H, W), dtype=bool)
        for bins in bins_list:
            bad |= _near_edge(vals, bins).any(axis=1)
        n = int(bad.sum())
        if n == 0:
            break
        fresh = (rng.standard_normal((n, C)) * scale).astype(F32)
        z.transpose(0, 2, 3, 1)[bad] = fresh
    assert n == 0 and rounds < 50, (n, rounds)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def region_case(name, shape, C, max_regions=64):
    """(target int64 [B,H,W], (labels, count, table)) for the region tests: "blobs" sparse squares on background, "full" one region of
    class max(C, 2) - 1 filling image 0, "noise" class noise that overflows a 64-row table (where the image has room for it)."""
    B, H, W = shape
    top = max(C, 2) - 1
    if name == "blobs":
        rng = np.random.default_rng(H + W)
        t = np.zeros(shape, dtype=np.int64)
        for b in range(B):
            for _ in range(6):
                y, x, h, w = rng.integers(0, H), rng.integers(0, W), rng.integers(1, 9), rng.integers(1, 9)
                t[b, y:y + h, x:x + w] = rng.integers(1, top + 1)
    elif name == "full":
        t = R.noise(B, H, W, 0.1, top + 1, seed=H)
        t[0] = top
    elif name == "noise":
        t = R.noise(B, H, W, 0.3, top + 1, seed=W)
    else:
        raise KeyError(name)
    t = np.ascontiguousarray(t)
    return t, R.label_batch(t, (), 8, 0, 1, max_regions)
