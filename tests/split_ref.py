"""The reference of the split tests (tests/test_split_host.py, tests/test_gpu_split.py), independent of the union-find and of the round
scheme of the package: per source label the markers by scipy.ndimage.label, per marker the geodesic distance inside the defect by
repeated ndimage.binary_dilation(..., mask=defect) stopped at max_iters, every pixel to the marker at the least (distance, first
pixel), the pieces by ndimage.label per code and the numbering and tables by the brute-force rules of tests/instances_ref.py.

Why the flood restates the rounds, also when max_iters cuts them short: a pixel at geodesic distance d from its nearest marker has no
owned neighbour before round d (every neighbour is at distance >= d - 1 and is owned from its own distance on), and in round d its
owned neighbours are exactly those at distance d - 1, each owned (by induction) by the lowest marker at distance d - 1 from it; the
markers at distance d from the pixel are the union of those sets, so the smallest owner among the neighbours is the lowest marker at
distance d.  A pixel farther than max_iters from every marker of its defect stays unowned.  Every comparison built on this is exact."""
import functools

import numpy as np
import torch
from scipy import ndimage

import instances_ref as IR

FAR = np.int64(2 ** 40)
NO_FEATURE = 2 ** 30
D2 = 25                       # the table's marker radius 5: every generated image splits a defect (d2 = 9, 16: the comparisons)
INFORMATIVE = 37              # the generator's claims are made from this extent on: a disc pair with cores needs a dozen rows


def distance_sq(labels):
    """int32 [B,H,W]: the squared Euclidean distance to the nearest pixel of no component; NO_FEATURE where an image has none."""
    out = np.empty(labels.shape, dtype=np.int32)
    for b, lab in enumerate(labels):
        fg = lab != 0
        out[b] = NO_FEATURE if fg.all() else np.rint(ndimage.distance_transform_edt(fg) ** 2).astype(np.int32)
    return out


def owners(lab, marker, connectivity, min_marker_area, max_iters):
    """One image: (owner int64 [H,W], converged, ties bool [H,W]: pixels with two nearest markers at one distance)."""
    st = IR.S8 if connectivity == 8 else IR.S4
    own = np.zeros(lab.shape, dtype=np.int64)
    best = np.full(lab.shape, FAR)
    ties = np.zeros(lab.shape, dtype=bool)
    seeded = np.zeros(lab.shape, dtype=bool)        # the defects that hold a surviving marker
    for l in np.unique(lab[lab > 0]):
        defect = lab == l
        mlab, n = ndimage.label(defect & marker, structure=st)
        for k in range(1, n + 1):                   # scipy numbers by first pixel: ascending ids
            mk = mlab == k
            if mk.sum() < min_marker_area:
                continue
            ident = int(np.flatnonzero(mk)[0]) + 1
            dist = np.full(lab.shape, FAR)
            dist[mk] = 0
            cur, d = mk, 0
            while d < max_iters:
                nxt = ndimage.binary_dilation(cur, structure=st, mask=defect)
                new = nxt & ~cur
                if not new.any():
                    break
                d += 1
                dist[new] = d
                cur = nxt
            ties |= (dist == best) & (dist < FAR)
            better = dist < best                    # strict: of equal distances the lower first pixel stays
            own[better], best[better] = ident, dist[better]
            ties &= ~better
            seeded |= defect
    return own, not (seeded & (own == 0)).any(), ties


def split_batch(labels, src_table, marker, maps=(), connectivity=8, min_marker_area=1, max_iters=256, min_area=1, max_instances=None):
    """labels int32 [B,H,W], src_table int64 [B,Ms,9], marker bool [B,H,W], maps float32 [B,H,W] arrays -> dict of labels, count,
    table, parent, pieces, converged (as split_instances returns them) and owner, ties."""
    B, Ms = labels.shape[0], src_table.shape[1]
    M = Ms if max_instances is None else max_instances
    out = {k: [] for k in ("labels", "count", "table", "parent", "pieces", "converged", "owner", "ties")}
    for b in range(B):
        lab = labels[b].astype(np.int64)
        own, conv, ties = owners(lab, marker[b], connectivity, min_marker_area, max_iters)
        code = np.where(lab > 0, lab * 2 ** 32 + own, 0)
        plab, count, table = IR.label_image(code, [v[b] for v in maps], connectivity, 0, min_area, M)
        n = min(count, M)
        src = table[:n, 0] // 2 ** 32
        parent = np.zeros(M, dtype=np.int32)
        parent[:n] = src
        table[:n, 0] = [src_table[b, s - 1, 0] if s <= Ms else -1 for s in src]
        pieces = np.array([(parent == s).sum() for s in range(1, Ms + 1)], dtype=np.int32)
        for k, v in zip(out, (plab, count, table, parent, pieces, conv, own, ties)):
            out[k].append(v)
    res = {k: np.stack(v) if k not in ("count", "converged") else np.array(v) for k, v in out.items()}
    res["count"] = res["count"].astype(np.int32)
    return res


# ------------------------------------------------------------------------------------------------ generated cases
def _disc(m, cy, cx, r, value):
    H, W = m.shape
    y, x = np.mgrid[0:H, 0:W]
    m[(y - cy) ** 2 + (x - cx) ** 2 <= r * r] = value


def disc_pairs(H, W, seed):
    """(mask int64 [H,W], centres bool [H,W]): pairs of overlapping discs of classes 1..3 (radii 5..9, centre distance r .. 2r - 2,
    some partly outside the frame; later pairs overwrite earlier ones, so classes touch), isolated discs of radius 2 (no core at
    d2 = 25) and salt on the background.  centres: a 3 x 3 block on every disc centre of a pair, single pixels on the small discs."""
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), dtype=np.int64)
    centres = np.zeros((H, W), dtype=bool)
    n = max(1, H * W // 700)
    for _ in range(n):
        r = int(rng.integers(5, 10))
        cy, cx = rng.uniform(-2, H + 2), rng.uniform(-2, W + 2)
        d, th = rng.uniform(r, 2 * r - 2), rng.uniform(0, 2 * np.pi)
        c = int(rng.integers(1, 4))
        for py, px in ((cy, cx), (cy + d * np.sin(th), cx + d * np.cos(th))):
            _disc(m, py, px, r, c)
        for py, px in ((cy, cx), (cy + d * np.sin(th), cx + d * np.cos(th))):
            iy, ix = int(round(py)), int(round(px))
            centres[max(iy - 1, 0):max(iy + 2, 0), max(ix - 1, 0):max(ix + 2, 0)] = True
    for _ in range(n):
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        if not m[max(cy - 4, 0):cy + 5, max(cx - 4, 0):cx + 5].any():
            _disc(m, cy, cx, 2, int(rng.integers(1, 4)))
            centres[cy, cx] = True
    salt = (rng.random((H, W)) < 0.004) & (m == 0)
    m[salt] = rng.integers(1, 4, (H, W))[salt]
    return m, centres


class Case:
    """One generated batch and what every test of it shares: the source labelling by tests/instances_ref.py (not by the package)."""

    def __init__(self, B, H, W, connectivity, seed=0):
        parts = [disc_pairs(H, W, seed * 100 + b) for b in range(B)]
        self.mask = np.stack([p[0] for p in parts])
        self.centres = np.stack([p[1] for p in parts])
        self.connectivity = connectivity
        self.maps = IR.random_maps(B, H, W, seed=seed + 5)
        self.labels, self.count, self.table = IR.label_batch(self.mask, (), connectivity, 0, 1, 256)
        assert self.count.max() <= 256
        self.distance = distance_sq(self.labels)

    def inst(self, device="cpu"):
        from uaps_amd.instances import InstanceResult
        return InstanceResult(torch.from_numpy(self.labels).to(device), torch.from_numpy(self.count).to(device),
                              torch.from_numpy(self.table).to(device), 0)

    def marker(self, form):
        return self.distance >= D2 if form == "distance" else self.centres

    @functools.lru_cache(maxsize=None)
    def expected(self, form, min_marker_area=1, max_iters=256, min_area=1, max_instances=None, with_maps=True, check=True):
        ref = split_batch(self.labels, self.table, self.marker(form), self.maps if with_maps else (), self.connectivity,
                          min_marker_area, max_iters, min_area, max_instances)
        if check and min_marker_area == 1 and min_area == 1 and max_instances is None and min(self.mask.shape[1:]) >= INFORMATIVE:
            assert_informative(self, ref, form)
        return ref


def assert_informative(case, ref, form):
    """The case shows something: a defect cut in two or more, a defect without a marker kept whole, a pixel with two nearest markers at
    one distance, and a piece labelling that differs from the source's."""
    assert ref["converged"].all()
    assert (ref["pieces"] >= 2).any(), "no defect is split"
    marker = case.marker(form)
    whole = False
    for b in range(case.labels.shape[0]):
        held = np.unique(case.labels[b][marker[b] & (case.labels[b] > 0)])
        bare = np.setdiff1d(np.arange(1, case.count[b] + 1), held)
        whole |= len(bare) > 0 and (ref["pieces"][b][bare - 1] == 1).all()
    assert whole, "every defect holds a marker"
    assert ref["ties"].any(), "no pixel has two nearest markers at one distance"
    assert not np.array_equal(ref["labels"], case.labels)


@functools.lru_cache(maxsize=None)
def case(B, H, W, connectivity, seed=0):
    return Case(B, H, W, connectivity, seed)


def assert_equal(res, ref, what=""):
    """res: a uaps_amd SplitResult; ref: split_batch's dict.  Bit for bit."""
    IR.assert_equal(res.instances, (ref["labels"], ref["count"], ref["table"]), what)
    assert res.parent.dtype == torch.int32 and np.array_equal(res.parent.cpu().numpy(), ref["parent"]), what
    assert res.pieces.dtype == torch.int32 and np.array_equal(res.pieces.cpu().numpy(), ref["pieces"]), what
    assert res.converged.dtype == torch.bool and np.array_equal(res.converged.cpu().numpy(), ref["converged"]), what


# ------------------------------------------------------------------------------------------------ hand-made inputs
def source(mask, connectivity=8, device="cpu", max_instances=256, min_area=1):
    """mask int64 [B,H,W] array -> (InstanceResult on `device`, labels, table) by tests/instances_ref.py."""
    from uaps_amd.instances import InstanceResult
    labels, count, table = IR.label_batch(mask, (), connectivity, 0, min_area, max_instances)
    return InstanceResult(torch.from_numpy(labels).to(device), torch.from_numpy(count).to(device),
                          torch.from_numpy(table).to(device), 0), labels, table


def chain_ends(m):
    """bool [1,H,W]: the two end pixels (one 8-neighbour) of a one-pixel-wide open chain such as IR.spiral or IR.comb."""
    fg = m[0] != 0
    nb = ndimage.convolve(fg.astype(int), np.ones((3, 3), dtype=int), mode="constant") - 1
    ends = fg & (nb == 1)
    assert ends.sum() == 2
    return ends[None]
