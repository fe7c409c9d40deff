"""Defect instances and run-length masks on the kernels of csrc/instances.hip.

`label_instances` turns a class mask into a list of defects: connected components per class, numbered per image by their first pixel
in raster order (scipy.ndimage.label's order), with a per-defect table -- class, area, half-open bounding box, first pixel and the
exact fixed-point sums of up to two maps (confidence, uncertainty) over the component.  Nothing in it synchronises with the host;
`InstanceResult.records()` is the one device-to-host copy.

`mask_to_rle` / `rle_to_mask` are the reference's run-length exchange format (utilities/utilities.py:36-63, mask2rle / make_mask) as
device ops, `format_rle` / `parse_rle` its string form on the host: pairs "start length" over the column-major walk of a binary plane,
1-based starts, single spaces, the empty string for an empty plane.

CPU tensors take the numpy restatements below (a two-pass union-find; no scipy), as in the other modules; on a ROCm device a missing
kernel is an error."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._checks import TOO_BIG as _TOO_BIG

TABLE_COLUMNS = ("class", "area", "y0", "x0", "y1", "x1", "first_pixel", "sum0", "sum1")
FIXED_ONE = 16777216.0                   # 2^24: q(v) = (int64) rint(clamp(v, -65536, 65536) * 2^24)
_ws = _lib.Workspace()


class InstanceResult(NamedTuple):
    """labels: int32 [B,H,W], 0 = background or removed; count: int32 [B], the true number of components after filtering;
    table: int64 [B,max_instances,9], columns TABLE_COLUMNS, rows from count[b] on are zero; n_maps: how many sum columns are filled."""
    labels: torch.Tensor
    count: torch.Tensor
    table: torch.Tensor
    n_maps: int = 0

    @property
    def max_instances(self) -> int:
        return self.table.shape[1]

    @property
    def overflow(self) -> torch.Tensor:
        """bool [B]: more components than rows."""
        return self.count > self.max_instances

    def means(self) -> torch.Tensor:
        """float64 [B,max_instances,2]: sum / 2^24 / area; 0 in rows without a component."""
        area = self.table[..., 1:2].to(torch.float64)
        s = self.table[..., 7:9].to(torch.float64) / FIXED_ONE
        return torch.where(area > 0, s / area.clamp(min=1.0), torch.zeros_like(s))

    def records(self) -> List[List[dict]]:
        """One device-to-host copy; per image a list of dicts label, cls, area, bbox (y0, x0, y1, x1), mean0, mean1 (None for a map
        that was not passed)."""
        B, M = self.table.shape[:2]
        packed = torch.cat([self.table.reshape(B, -1), self.count.to(torch.int64).reshape(B, 1)], dim=1).cpu().numpy()
        out = []
        for b in range(B):
            rows, n = packed[b, :-1].reshape(M, 9), int(packed[b, -1])
            recs = []
            for k in range(min(n, M)):
                r = rows[k]
                area = int(r[1])
                means = [float(r[7 + j]) / FIXED_ONE / area if j < self.n_maps else None for j in range(2)]
                recs.append({"label": k + 1, "cls": int(r[0]), "area": area, "bbox": (int(r[2]), int(r[3]), int(r[4]), int(r[5])),
                             "mean0": means[0], "mean1": means[1]})
            out.append(recs)
        return out


def host_tables(table: torch.Tensor, inst: InstanceResult) -> Tuple[np.ndarray, np.ndarray]:
    """One device-to-host copy of a descriptor table [B,M,K] packed beside the instance table: (int64 [B,M,K], int64 [B,M,9])."""
    B, M, K = table.shape
    packed = torch.cat([table.reshape(B, -1), inst.table.reshape(B, -1)], dim=1).cpu().numpy()
    return packed[:, :M * K].reshape(B, M, K), packed[:, M * K:].reshape(B, M, 9)


def add_props(records: List[List[dict]], props) -> List[List[dict]]:
    """Every key of a props() dict (arrays [B,max_instances]) added to each defect's dict of records(), in place."""
    for b, rows in enumerate(records):
        for r in rows:
            k = r["label"] - 1
            for name, arr in props.items():
                r[name] = float(arr[b, k])
    return records


def fixed_point(v: np.ndarray) -> np.ndarray:
    """q(v) of the table's sums on the host: int64, NaN -> 0.  Scaling by 2^24 is exact in fp32 and the product is below 2^41."""
    v = np.asarray(v, dtype=np.float32)
    c = np.clip(np.where(np.isnan(v), np.float32(0), v), np.float32(-65536), np.float32(65536)).astype(np.float32)
    return np.rint(c * np.float32(FIXED_ONE)).astype(np.int64)


def _find(parent, a):
    while parent[a] != a:
        a = parent[a]
    return a


def _label_image(m: np.ndarray, conn8: bool, background):
    """Two-pass union-find over one image: roots int64 [H*W], the smallest raster index of every pixel's component (-1: background)."""
    H, W = m.shape
    flat = m.reshape(-1).tolist()
    parent = list(range(H * W))
    fg = [background is None or v != background for v in flat]
    for y in range(H):
        for x in range(W):
            i = y * W + x
            if not fg[i]:
                continue
            c = flat[i]
            back = [i - 1] if x > 0 else []
            if y > 0:
                back.append(i - W)
                if conn8:
                    if x > 0:
                        back.append(i - W - 1)
                    if x < W - 1:
                        back.append(i - W + 1)
            for j in back:
                if fg[j] and flat[j] == c:
                    ra, rb = _find(parent, i), _find(parent, j)
                    if ra != rb:
                        lo, hi = (ra, rb) if ra < rb else (rb, ra)
                        parent[hi] = lo
                    parent[i] = min(ra, rb)
    roots = np.empty(H * W, dtype=np.int64)
    for i in range(H * W):
        if fg[i]:
            r = _find(parent, i)
            parent[i] = r
            roots[i] = r
        else:
            roots[i] = -1
    return roots


def _label_cpu(mask, maps, connectivity, background, min_area, max_instances) -> InstanceResult:
    m = mask.numpy()
    B, H, W = m.shape
    labels = np.zeros((B, H * W), dtype=np.int32)
    count = np.zeros(B, dtype=np.int32)
    table = np.zeros((B, max_instances, 9), dtype=np.int64)
    qs = [fixed_point(t.numpy()).reshape(B, -1) for t in maps]
    for b in range(B):
        roots = _label_image(m[b], connectivity == 8, background)
        idx = np.nonzero(roots >= 0)[0]
        area = np.bincount(roots[idx], minlength=H * W)
        keep = np.nonzero(area >= min_area)[0]              # ascending root = ascending first pixel
        number = np.zeros(H * W, dtype=np.int64)
        number[keep] = np.arange(1, len(keep) + 1)
        lab = np.zeros(H * W, dtype=np.int64)
        lab[idx] = number[roots[idx]]
        labels[b] = lab
        count[b] = len(keep)
        sel = np.nonzero((lab > 0) & (lab <= max_instances))[0]
        k = lab[sel] - 1
        n = min(len(keep), max_instances)
        t = table[b]
        t[:n, 0] = m[b].reshape(-1)[keep[:n]]
        t[:n, 1] = area[keep[:n]]
        t[:n, 2], t[:n, 3] = H, W
        t[:n, 6] = keep[:n]
        ys, xs = sel // W, sel % W
        np.minimum.at(t[:, 2], k, ys)
        np.minimum.at(t[:, 3], k, xs)
        np.maximum.at(t[:, 4], k, ys + 1)
        np.maximum.at(t[:, 5], k, xs + 1)
        for j, q in enumerate(qs):
            np.add.at(t[:, 7 + j], k, q[b][sel])
    return InstanceResult(torch.from_numpy(labels.reshape(B, H, W)), torch.from_numpy(count), torch.from_numpy(table), len(maps))


def label_instances(mask: torch.Tensor, maps: Sequence[torch.Tensor] = (), *, connectivity: int = 8, background: Optional[int] = 0,
                    min_area: int = 1, max_instances: int = 256) -> InstanceResult:
    """Connected components of the int64 class mask [B,H,W] (what argmax, predict and TTAResult.mask produce) and their table.
    maps: zero, one or two float32 [B,H,W] tensors summed (fixed point, exact) over each component.  background=None: every class
    forms components.  Components below min_area pixels get label 0 and no row; the others are numbered 1..N_b by their first pixel
    in raster order.  labels and count are complete whatever max_instances is; the table holds the first max_instances components."""
    if isinstance(maps, torch.Tensor):
        maps = (maps,)
    maps = tuple(maps)
    if mask.dim() != 3 or mask.dtype != torch.int64:
        raise TypeError("label_instances: int64 [B,H,W] class mask expected")
    if len(maps) > 2:
        raise ValueError("label_instances: at most two maps")
    for t in maps:
        if t.dtype != torch.float32 or t.shape != mask.shape or t.device != mask.device:
            raise TypeError("label_instances: maps are float32 [B,H,W] tensors on the mask's device")
    if connectivity not in (4, 8):
        raise ValueError("label_instances: connectivity is 4 or 8")
    min_area, max_instances = int(min_area), int(max_instances)
    if min_area < 1 or max_instances < 1:
        raise ValueError("label_instances: min_area >= 1 and max_instances >= 1")
    B, H, W = mask.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError("label_instances: empty mask")
    if H * W >= _TOO_BIG or B * H * W * 8 >= _TOO_BIG or B * max_instances * 72 >= _TOO_BIG:
        raise ValueError("label_instances: H*W < 2^31, B*H*W*8 < 2 GiB and a table below 2 GiB")
    if not mask.is_cuda:
        return _label_cpu(mask.detach().contiguous(), [t.detach().contiguous() for t in maps], connectivity,
                          None if background is None else int(background), min_area, max_instances)
    dev = mask.device
    mask = mask.detach().contiguous()
    maps = [t.detach().contiguous() for t in maps]
    labels = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    table = torch.empty((B, max_instances, 9), dtype=torch.int64, device=dev)
    _lib.call("uaps_label_instances", _lib.InstancesCall, dev, _ws, _lib.workspace_bytes("uaps_instances_workspace_bytes", B, H, W),
              B=B, H=H, W=W, connectivity=connectivity, has_background=0 if background is None else 1,
              background=0 if background is None else int(background), min_area=min_area, max_instances=max_instances,
              mask=mask.data_ptr(), map0=maps[0].data_ptr() if len(maps) > 0 else None, map1=maps[1].data_ptr() if len(maps) > 1 else None,
              labels=labels.data_ptr(), count=count.data_ptr(), table=table.data_ptr())
    return InstanceResult(labels, count, table, len(maps))


# ------------------------------------------------------------------------------------------------ run-length masks
class RLE(NamedTuple):
    """CSR runs of B images x len(classes) classes: pairs int32 [R,2] (1-based column-major start, length), offsets int32
    [B*len(classes)+1]; segment b * len(classes) + c holds the runs of classes[c] in image b."""
    pairs: torch.Tensor
    offsets: torch.Tensor
    shape: Tuple[int, int]
    classes: Tuple[int, ...]

    def segment(self, b: int, c: int) -> torch.Tensor:
        """The [n,2] pairs of image b and class index c (a device-to-host read of two offsets)."""
        j = b * len(self.classes) + c
        lo, hi = (int(v) for v in self.offsets[j:j + 2].tolist())
        return self.pairs[lo:hi]


def _check_classes(classes) -> Tuple[int, ...]:
    classes = tuple(int(c) for c in classes)
    if not 1 <= len(classes) <= _lib.RLE_MAX_CLASSES or len(set(classes)) != len(classes):
        raise ValueError(f"1..{_lib.RLE_MAX_CLASSES} distinct classes")
    return classes


def _plane_runs(plane: np.ndarray) -> np.ndarray:
    """The runs of one binary plane [H,W] over its column-major walk: int32 [n,2] of (1-based start, length)."""
    walk = np.zeros(plane.size + 2, dtype=np.int8)
    walk[1:-1] = plane.reshape(-1, order="F")
    step = np.diff(walk)
    starts, ends = np.flatnonzero(step == 1), np.flatnonzero(step == -1)
    return np.stack([starts + 1, ends - starts], axis=1).astype(np.int32)


def mask_to_rle(mask: torch.Tensor, classes: Sequence[int]) -> RLE:
    """The runs of every (image, class) of a label array [B,H,W] (int64, or the uint8 arrays the input pipelines keep).  Two passes on
    the device -- count and scan, then write -- with one host read of the total between them, which sizes `pairs`."""
    classes = _check_classes(classes)
    if mask.dim() != 3 or mask.dtype not in (torch.int64, torch.uint8):
        raise TypeError("mask_to_rle: int64 or uint8 [B,H,W] expected")
    B, H, W = mask.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError("mask_to_rle: empty mask")
    if H * W >= _TOO_BIG or B * H * W * 8 >= _TOO_BIG:
        raise ValueError("mask_to_rle: H*W < 2^31 and B*H*W*8 < 2 GiB")
    if not mask.is_cuda:
        m = mask.numpy()
        segs = [_plane_runs(m[b] == c) for b in range(B) for c in classes]
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int32)
        pairs = np.concatenate(segs).reshape(-1, 2) if segs else np.zeros((0, 2), np.int32)
        return RLE(torch.from_numpy(pairs), torch.from_numpy(offsets), (H, W), classes)
    dev = mask.device
    mask = mask.detach().to(torch.int64).contiguous()
    n = B * len(classes) * W
    col = torch.empty((n + 1,), dtype=torch.int32, device=dev)
    fields = dict(B=B, H=H, W=W, n_classes=len(classes), classes=classes, mask=mask.data_ptr(), col_offsets=col.data_ptr())
    _lib.call("uaps_rle_count", _lib.RleCall, dev, **fields)
    total = int(col[n])                                     # the one synchronisation: the size of the result
    pairs = torch.empty((total, 2), dtype=torch.int32, device=dev)
    if total:
        _lib.call("uaps_rle_encode", _lib.RleCall, dev, pairs=pairs.data_ptr(), **fields)
    offsets = col[::W].contiguous()
    return RLE(pairs, offsets, (H, W), classes)


def rle_to_mask(pairs: torch.Tensor, offsets: torch.Tensor, shape: Tuple[int, int], classes: Sequence[int],
                dtype: torch.dtype = torch.int64) -> torch.Tensor:
    """The inverse (make_mask's inner loop for any H, W): a zero label array [B,H,W] (int64 or uint8) in which the pixels
    [start-1, start-1+length) of the column-major walk receive the class of their segment; later classes win on overlap."""
    classes = _check_classes(classes)
    H, W = int(shape[0]), int(shape[1])
    if dtype not in (torch.int64, torch.uint8):
        raise TypeError("rle_to_mask: int64 or uint8 output")
    if dtype == torch.uint8 and any(c < 0 or c > 255 for c in classes):
        raise ValueError("rle_to_mask: a class outside [0, 255] does not fit a uint8 label array")
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int32 or offsets.dtype != torch.int32 or offsets.dim() != 1:
        raise TypeError("rle_to_mask: int32 [R,2] pairs and int32 offsets expected")
    segs = offsets.numel() - 1
    if H < 1 or W < 1 or segs < 1 or segs % len(classes):
        raise ValueError("rle_to_mask: offsets hold B * len(classes) + 1 entries")
    B = segs // len(classes)
    if H * W >= _TOO_BIG or B * H * W * 8 >= _TOO_BIG:
        raise ValueError("rle_to_mask: H*W < 2^31 and B*H*W*8 < 2 GiB")
    if not pairs.is_cuda:
        p, o = pairs.numpy(), offsets.numpy()
        _check_runs(p, H * W)
        out = np.zeros((B, H * W), dtype=np.int64)
        for b in range(B):
            for k, c in enumerate(classes):
                j = b * len(classes) + k
                for s, n in p[o[j]:o[j + 1]]:
                    out[b, s - 1:s - 1 + n] = c
        return torch.from_numpy(out.reshape(B, W, H).transpose(0, 2, 1).copy()).to(dtype)
    dev = pairs.device
    pairs, offsets = pairs.contiguous(), offsets.to(dev).contiguous()
    out = torch.empty((B, H, W), dtype=dtype, device=dev)
    _lib.call("uaps_rle_decode", _lib.RleCall, dev, B=B, H=H, W=W, n_classes=len(classes), classes=classes,
              pairs=pairs.data_ptr() if pairs.shape[0] else None, offsets=offsets.data_ptr(), n_runs=pairs.shape[0], out=out.data_ptr(),
              out_uint8=1 if dtype == torch.uint8 else 0)
    return out


def _check_runs(p: np.ndarray, plane: int) -> None:
    if len(p) and (p[:, 0].min() < 1 or p[:, 1].min() < 0 or (p[:, 0].astype(np.int64) - 1 + p[:, 1]).max() > plane):
        raise ValueError(f"a run leaves the plane of {plane} pixels")


def format_rle(pairs) -> str:
    """One CSR slice ([n,2] pairs, tensor or array) as the reference's string: "start length start length ..."."""
    p = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
    return " ".join(str(int(v)) for v in p.reshape(-1))


def parse_rle(text: str, shape: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """The string form -> int32 [n,2] pairs on the host.  With `shape` (H, W) a run that leaves the plane is a ValueError, here,
    before anything is launched."""
    fields = text.split()
    if len(fields) % 2:
        raise ValueError("parse_rle: an odd number of fields")
    try:
        p = np.array([int(f) for f in fields], dtype=np.int64).reshape(-1, 2)
    except ValueError as e:
        raise ValueError(f"parse_rle: {e}") from None
    if len(p) and (p.min() < 0 or p.max() >= _TOO_BIG):
        raise ValueError("parse_rle: a field outside [0, 2^31)")
    if shape is not None:
        _check_runs(p, int(shape[0]) * int(shape[1]))
    elif len(p) and p[:, 0].min() < 1:
        raise ValueError("parse_rle: starts are 1-based")
    return torch.from_numpy(p.astype(np.int32))


def rle_from_strings(strings: Sequence[Sequence[str]], shape: Tuple[int, int], classes: Sequence[int], device=None) -> RLE:
    """strings[b][c]: the annotation of class classes[c] in image b ("" or None: none) -> the CSR form rle_to_mask takes, on `device`.
    Every run is checked against the plane on the host."""
    classes = _check_classes(classes)
    segs = []
    for row in strings:
        if len(row) != len(classes):
            raise ValueError("rle_from_strings: one string per class and image")
        segs += [parse_rle(s or "", shape) for s in row]
    offsets = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in segs])]), dtype=torch.int32)
    pairs = torch.cat(segs) if segs else torch.zeros((0, 2), dtype=torch.int32)
    if device is not None:
        pairs, offsets = pairs.to(device), offsets.to(device)
    return RLE(pairs, offsets, (int(shape[0]), int(shape[1])), classes)
