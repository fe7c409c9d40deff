"""On-device input pipelines for every dataset recipe of the reference and for UCC's weak / strong views
(csrc/augment_views.hip, include/uaps_hip.h: uaps_augment_views).

`augment.py` / csrc/augment.hip build one pipeline, the NEU recipe on 3-channel sources.  The other loaders of the reference run
the same stages in other orders, on one channel (DAGM), to a rectangular output (KoSDD2), or add GridDistortion, ColorJitter and
PixelDropout and want two differently augmented views of one image (UCC).  Here a `Recipe` holds the stage list as data,
`draw` turns it into one program per image, and `augment_views` launches the interpreting gather kernel once for one or two views (the UCC source launches it once per
view: measured 4 % faster).

PARITY UNPINNED: cv2 and albumentations are not in the build image and the reference ships no image fixtures.  The settings
below restate the reference's calls (file:line beside each recipe) with albumentations' documented defaults where the reference
passes nothing -- RandomBrightnessContrast p = 0.5, Blur blur_limit = 7 (odd k in {3, 5, 7}), GaussNoise var_limit = (10, 50),
GridDistortion num_steps = 5 / distort_limit = 0.3 / bilinear / reflect-101 -- and the arithmetic is the one include/uaps_hip.h
writes down.  Nothing here is a measured equality with either library.  The draws come from a numpy Generator the caller owns:
same distributions as albumentations, not its random sequence.

Geometry (resize, flips, quarter turns) is always applied first; every other stage runs in the order of the recipe.  For the NEU
recipe, whose quarter turn sits between Blur and GaussNoise, this is the same image: the turn commutes with the pointwise
brightness / contrast table and with the symmetric box window.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterator, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .augment import IMAGENET_MEAN, IMAGENET_STD

ROW_DTYPE = np.dtype([("hflip", np.int32), ("vflip", np.int32), ("rot_k", np.int32), ("grid_on", np.int32),
                      ("op", np.int32, (_lib.AUG_MAX_OPS,)), ("a", np.float32, (_lib.AUG_MAX_OPS,)),
                      ("b", np.float32, (_lib.AUG_MAX_OPS,))])
assert ROW_DTYPE.itemsize == C.sizeof(_lib.ViewRow)

OPS = {"bc": _lib.AUG_BC, "noise": _lib.AUG_NOISE, "blur": _lib.AUG_BLUR, "bright": _lib.AUG_BRIGHT, "contrast": _lib.AUG_CONTRAST,
       "saturate": _lib.AUG_SATURATE, "hue": _lib.AUG_HUE, "pixdrop": _lib.AUG_PIXDROP, "grid": _lib.AUG_GRID}
GRID_STEPS, GRID_LIMIT = 5, 0.3                 # A.GridDistortion defaults
DAGM_MEAN, DAGM_STD = (0.5314,), (0.1357,)      # DAGM-Dataset-codes/UAPS_dataloaders.py:94-95


class Stage(NamedTuple):
    """One albumentations transform: kind in hflip / vflip / rot90 / bc / blur / noise / grid / jitter / pixdrop, its probability
    and its ranges."""
    kind: str
    p: float
    lo: float = 0.0
    hi: float = 0.0


class Recipe(NamedTuple):
    name: str
    out_size: Tuple[int, int]                  # (Ho, Wo) of A.Resize(Ho, Wo, INTER_NEAREST)
    stages: Tuple[Stage, ...]
    mean: Tuple[float, ...] = IMAGENET_MEAN
    std: Tuple[float, ...] = IMAGENET_STD


def _bc(p=0.5):            # A.RandomBrightnessContrast((0, 0.5), (0, 0.5)): both limits in lo..hi
    return Stage("bc", p, 0.0, 0.5)


def _noise(p):             # A.GaussNoise: var_limit (10, 50)
    return Stage("noise", p, 10.0, 50.0)


def _blur(p):              # A.Blur: blur_limit 7 -> odd k in 3..7
    return Stage("blur", p, 3, 7)


RECIPES = {r.name: r for r in (
    # utilities/dataloaders.py:98-102
    Recipe("neu", (256, 256), (Stage("hflip", 0.4), Stage("vflip", 0.4), _bc(), _blur(0.3), Stage("rot90", 0.3), _noise(0.3))),
    # DAGM-Dataset-codes/UAPS_dataloaders.py:97-100 (t_train) and :102-105 (t_untrain): 1-channel sources, noise first
    Recipe("dagm_labelled", (256, 256), (Stage("hflip", 0.3), Stage("vflip", 0.3), _noise(0.3), _bc(), _blur(0.2)), DAGM_MEAN, DAGM_STD),
    Recipe("dagm_unlabelled", (256, 256), (Stage("hflip", 0.4), Stage("vflip", 0.3), _noise(0.3), _bc(), _blur(0.3)), DAGM_MEAN, DAGM_STD),
    # KoSDD2-Dataset-Codes/UAPS_dataloaders.py:107-111
    Recipe("kosdd2", (512, 256), (Stage("hflip", 0.3), Stage("vflip", 0.3), _bc(), _blur(0.3), _noise(0.3))),
    # MTiles-Dataset-codes/UAPS_dataloaders.py:96-99
    Recipe("mtiles", (256, 256), (Stage("hflip", 0.5), Stage("vflip", 0.5), _bc(), _blur(0.3), _noise(0.4))),
    # UCC/UCC_dataloaders.py:149-154 (t_train), :156-160 (t_untrain_weak), :162-168 (t_untrain_strong)
    Recipe("ucc_labelled", (256, 256), (Stage("hflip", 0.3), Stage("vflip", 0.3), _bc(0.3), Stage("grid", 0.2, -GRID_LIMIT, GRID_LIMIT),
                                        _blur(0.3), _noise(0.4))),
    Recipe("ucc_weak", (256, 256), (_bc(0.3), _blur(0.3), _noise(0.4))),
    Recipe("ucc_strong", (256, 256), (_blur(0.3), Stage("jitter", 0.3, 0.2, 0.2), Stage("pixdrop", 0.2, 0.01, 0.01), _noise(0.4))),
    # t_val / t_test of every loader: A.Resize only
    Recipe("resize_only", (256, 256), ()),
)}


def recipe(r: Union[str, Recipe]) -> Recipe:
    if isinstance(r, Recipe):
        return r
    if r not in RECIPES:
        raise ValueError(f"unknown recipe {r!r}; known: {sorted(RECIPES)}")
    return RECIPES[r]


class ViewDraws(NamedTuple):
    """One view's parameters for B images: rows (ROW_DTYPE [B]: geometry row + program) and, when a row has grid_on, the 1-D
    coordinate maps grid_ys [B, Ho], grid_xs [B, Wo] (float32 positions in the working frame; identity for rows without)."""
    rows: np.ndarray
    grid_ys: Optional[np.ndarray]
    grid_xs: Optional[np.ndarray]


def empty_rows(B: int) -> np.ndarray:
    return np.zeros(B, ROW_DTYPE)


def set_program(row, ops: Sequence[Tuple]) -> None:
    """Write (name or opcode, a[, b]) entries into one row; the rest of the program is END."""
    if len(ops) > _lib.AUG_MAX_OPS:
        raise ValueError(f"a program holds at most {_lib.AUG_MAX_OPS} ops")
    row["op"][:] = 0; row["a"][:] = 0; row["b"][:] = 0
    for i, e in enumerate(ops):
        row["op"][i] = OPS[e[0]] if isinstance(e[0], str) else int(e[0])
        row["a"][i] = e[1] if len(e) > 1 else 0.0
        row["b"][i] = e[2] if len(e) > 2 else 0.0
    row["grid_on"] = int(any(o == _lib.AUG_GRID for o in row["op"]))


def grid_map(n: int, steps: np.ndarray) -> np.ndarray:
    """The 1-D map of A.GridDistortion along an axis of n pixels: the axis is cut into len(steps) equal cells, cell i is
    stretched by steps[i], the positions are piecewise linear in between and normalised to start at 0 and end at n - 1."""
    steps = np.asarray(steps, np.float64)
    knots = np.linspace(0.0, n - 1.0, len(steps) + 1)
    pos = np.concatenate([[0.0], np.cumsum(steps)]) * ((n - 1.0) / steps.sum())
    pos[-1] = n - 1.0
    return np.interp(np.arange(n, dtype=np.float64), knots, pos).astype(np.float32)


def draw(rec: Union[str, Recipe], B: int, rng: np.random.Generator, out_size: Optional[Tuple[int, int]] = None) -> ViewDraws:
    """One draw of the recipe per image.  `out_size` overrides the recipe's (the grid maps are as long as the output)."""
    rec = recipe(rec)
    Ho, Wo = out_size if out_size is not None else rec.out_size
    rows = empty_rows(B)
    gys = gxs = None
    for b in range(B):
        ops = []
        for st in rec.stages:
            fired = rng.random() < st.p
            if not fired:
                continue
            if st.kind == "hflip":
                rows[b]["hflip"] = 1
            elif st.kind == "vflip":
                rows[b]["vflip"] = 1
            elif st.kind == "rot90":
                rows[b]["rot_k"] = int(rng.integers(0, 4))
            elif st.kind == "bc":                                    # alpha = 1 + contrast, beta = brightness (x 255: brightness_by_max)
                ops.append(("bc", 1.0 + rng.uniform(st.lo, st.hi), rng.uniform(st.lo, st.hi)))
            elif st.kind == "blur":
                ops.append(("blur", float(rng.choice(np.arange(int(st.lo), int(st.hi) + 1, 2)))))
            elif st.kind == "noise":
                ops.append(("noise", float(np.sqrt(rng.uniform(st.lo, st.hi)))))
            elif st.kind == "grid":
                if gys is None:
                    gys = np.tile(np.arange(Ho, dtype=np.float32), (B, 1))
                    gxs = np.tile(np.arange(Wo, dtype=np.float32), (B, 1))
                gxs[b] = grid_map(Wo, 1.0 + rng.uniform(st.lo, st.hi, GRID_STEPS))
                gys[b] = grid_map(Ho, 1.0 + rng.uniform(st.lo, st.hi, GRID_STEPS))
                ops.append(("grid",))
            elif st.kind == "jitter":                                # A.ColorJitter(0.2, 0.2, 0.2, 0.2): four factors, random order
                f = (("bright", rng.uniform(1 - st.lo, 1 + st.lo)), ("contrast", rng.uniform(1 - st.lo, 1 + st.lo)),
                     ("saturate", rng.uniform(1 - st.lo, 1 + st.lo)), ("hue", rng.uniform(-st.hi, st.hi)))
                ops.extend(f[i] for i in rng.permutation(4))
            elif st.kind == "pixdrop":
                ops.append(("pixdrop", st.lo))
            else:
                raise ValueError(f"recipe {rec.name}: unknown stage {st.kind!r}")
        set_program(rows[b], ops)
    return ViewDraws(rows, gys, gxs)


def check_program(row) -> Optional[str]:
    """Why the kernel has no form for this row's program (None: it has one) -- the rules of include/uaps_hip.h."""
    ops = []
    for o in row["op"]:
        if o == _lib.AUG_END:
            break
        ops.append(int(o))
    if ops.count(_lib.AUG_GRID) > 1 or ops.count(_lib.AUG_BLUR) > 1:
        return "more than one GRID or BLUR"
    if ops.count(_lib.AUG_CONTRAST) > 1:
        return "more than one CONTRAST"
    if _lib.AUG_GRID in ops:
        head = ops[:ops.index(_lib.AUG_GRID)]
        if _lib.AUG_NOISE in head or _lib.AUG_PIXDROP in head:
            return "NOISE or PIXDROP ahead of GRID"
        if _lib.AUG_BLUR in head:
            return "BLUR ahead of GRID"
    return None


_ws = _lib.Workspace()


def _build_call(images: torch.Tensor, masks: Optional[torch.Tensor], draws: Union[ViewDraws, Sequence[ViewDraws]],
                  out_size: Tuple[int, int] = (256, 256), mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD,
                  seed: int = 0, noise: Optional[torch.Tensor] = None, drop_u: Optional[torch.Tensor] = None, return_means: bool = False):
    """The validated uaps_augment_views_call of augment_views and the tensors it points into: (call, keep-alive, x, y, workspace)."""
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] not in (1, 3):
        raise ValueError("augment_views: images must be uint8 [B, H, W, 1 or 3]")
    views = [draws] if isinstance(draws, ViewDraws) else list(draws)
    V = len(views)
    if V not in (1, 2):
        raise ValueError("augment_views: one or two views expected")
    B, Hs, Ws, Cs = images.shape
    Ho, Wo = out_size
    dev = images.device
    if masks is not None and (masks.dtype != torch.uint8 or tuple(masks.shape) != (B, Hs, Ws) or masks.device != dev):
        raise ValueError("augment_views: masks must be uint8 [B, H, W] on the images' device")
    if len(mean) < Cs or len(std) < Cs:
        raise ValueError("augment_views: one mean and std per channel expected")
    for d in views:
        if d.rows.dtype != ROW_DTYPE or d.rows.shape != (B,):
            raise ValueError("augment_views: one parameter row per image expected")
    rows = np.ascontiguousarray(np.stack([d.rows for d in views]))
    if (rows["rot_k"] % 2 == 1).any() and Ho != Wo:
        raise ValueError("augment_views: quarter turns need a square output")
    for r in rows.reshape(-1):
        why = check_program(r)
        if why is not None:
            raise ValueError(f"augment_views: the kernel has no form for this program ({why})")
    _lib.require_device(images, "augment_views")
    gys = gxs = None
    if rows["grid_on"].any():
        ident_y, ident_x = np.tile(np.arange(Ho, dtype=np.float32), (B, 1)), np.tile(np.arange(Wo, dtype=np.float32), (B, 1))
        ys = [d.grid_ys if d.grid_ys is not None else ident_y for d in views]
        xs = [d.grid_xs if d.grid_xs is not None else ident_x for d in views]
        if any(a.shape != (B, Ho) for a in ys) or any(a.shape != (B, Wo) for a in xs):
            raise ValueError("augment_views: grid maps must be [B, Ho] and [B, Wo]")
        gys = torch.from_numpy(np.ascontiguousarray(np.stack(ys), np.float32)).to(dev)
        gxs = torch.from_numpy(np.ascontiguousarray(np.stack(xs), np.float32)).to(dev)
    if noise is not None:
        if tuple(noise.shape) != (V, B, Cs, Ho, Wo) or noise.dtype != torch.float32 or noise.device != dev:
            raise ValueError("augment_views: noise must be float32 [V, B, Cs, Ho, Wo] on the images' device")
        noise = noise.contiguous()
    if drop_u is not None:
        if tuple(drop_u.shape) != (V, B, Ho, Wo) or drop_u.dtype != torch.float32 or drop_u.device != dev:
            raise ValueError("augment_views: drop_u must be float32 [V, B, Ho, Wo] on the images' device")
        drop_u = drop_u.contiguous()
    images = images.contiguous()
    masks = masks.contiguous() if masks is not None else None
    rows_dev = torch.from_numpy(rows.view(np.uint8).reshape(-1)).to(dev)
    x = torch.empty((V, B, Cs, Ho, Wo), dtype=torch.float32, device=dev)
    y = torch.empty((V, B, Ho, Wo), dtype=torch.int64, device=dev) if masks is not None else None
    ws = None
    if (rows["op"] == _lib.AUG_CONTRAST).any() or return_means:
        n = C.c_size_t()
        _lib.check(_lib.lib().uaps_augment_views_workspace_bytes(V, B, Ho, Wo, C.byref(n)), "uaps_augment_views_workspace_bytes")
        ws = _ws.get(dev, n.value) if not return_means else torch.full((n.value,), 0, dtype=torch.uint8, device=dev)
    call = _lib.AugmentViewsCall()
    call.struct_size = C.sizeof(_lib.AugmentViewsCall)
    call.V, call.B, call.Hs, call.Ws, call.Cs, call.Ho, call.Wo = V, B, Hs, Ws, Cs, Ho, Wo
    call.images, call.masks = images.data_ptr(), masks.data_ptr() if masks is not None else None
    call.rows_host, call.rows = rows.ctypes.data, rows_dev.data_ptr()
    call.grid_ys, call.grid_xs = (gys.data_ptr(), gxs.data_ptr()) if gys is not None else (None, None)
    call.noise = noise.data_ptr() if noise is not None else None
    call.drop_u = drop_u.data_ptr() if drop_u is not None else None
    call.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    for c in range(Cs):
        call.mean[c], call.std[c] = float(mean[c]), float(std[c])
    call.out, call.out_mask = x.data_ptr(), y.data_ptr() if y is not None else None
    call.workspace, call.workspace_bytes = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)
    return call, (images, masks, rows, rows_dev, gys, gxs, noise, drop_u), x, y, ws


def augment_views(images: torch.Tensor, masks: Optional[torch.Tensor], draws: Union[ViewDraws, Sequence[ViewDraws]],
                  out_size: Tuple[int, int] = (256, 256), mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD,
                  seed: int = 0, noise: Optional[torch.Tensor] = None, drop_u: Optional[torch.Tensor] = None, return_means: bool = False):
    """images: uint8 [B, Hs, Ws, Cs] on the GPU, Cs in {1, 3}; masks: uint8 [B, Hs, Ws] on the GPU or None; draws: one ViewDraws
    (V = 1) or a sequence of one or two (V = 2: both views read the same sources, one launch).
    Returns (x [V, B, Cs, Ho, Wo] float32 normalised, y [V, B, Ho, Wo] int64 or None).  `noise` ([V, B, Cs, Ho, Wo] float32,
    already scaled by each image's sigma) and `drop_u` ([V, B, Ho, Wo] float32 uniforms) replace the in-kernel Philox draws.
    return_means: also the contrast means m [V, B] the pre-pass computed (-1 where a program has no CONTRAST)."""
    call, keep, x, y, ws = _build_call(images, masks, draws, out_size, mean, std, seed, noise, drop_u, return_means)
    dev = images.device
    with _lib.device_guard(dev):
        call.stream = _lib.current_stream(dev)
        rc = _lib.lib().uaps_augment_views(C.byref(call))
    _lib.check(rc, "uaps_augment_views")
    if return_means:
        V, B = call.V, call.B
        m = ws[:V * B * 4].view(torch.float32).reshape(V, B).clone()
        if not (keep[2]["op"] == _lib.AUG_CONTRAST).any():
            m.fill_(-1.0)
        return x, y, m
    return x, y


def _to_device_u8(a, device, what: str) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    if t.dtype != torch.uint8:
        raise ValueError(f"{what} must be uint8")
    return t.to(device).contiguous()


class ArrayBatches:
    """A re-iterable batch source over already decoded uint8 arrays (file decoding stays on the host, outside this package):
    images [N, Hs, Ws, Cs] and masks [N, Hs, Ws] are kept on the device; every batch is a shuffled index draw, one host draw of the
    recipe and one launch.  Yields (x [batch, Cs, Ho, Wo] float32, y [batch, Ho, Wo] int64) as SegTrainer.fit expects; the last
    short batch is dropped (the loss kernels want one batch size)."""

    def __init__(self, images_u8, masks_u8, rec: Union[str, Recipe], batch: int, out_size: Optional[Tuple[int, int]] = None,
                 mean: Optional[Sequence[float]] = None, std: Optional[Sequence[float]] = None, seed: int = 0, shuffle: bool = True,
                 device="cuda"):
        self.recipe = recipe(rec)
        self.device = torch.device(device)
        self.images = _to_device_u8(images_u8, self.device, "ArrayBatches: images")
        if self.images.dim() == 3:
            self.images = self.images.unsqueeze(-1).contiguous()                     # [N, H, W] grey -> one channel
        self.masks = _to_device_u8(masks_u8, self.device, "ArrayBatches: masks") if masks_u8 is not None else None
        N = self.images.shape[0]
        if not 0 < int(batch) <= N:
            raise ValueError("ArrayBatches: batch must be in 1..len(images)")
        if self.masks is not None and tuple(self.masks.shape) != tuple(self.images.shape[:3]):
            raise ValueError("ArrayBatches: masks must be [N, H, W] like the images")
        self.batch, self.shuffle = int(batch), bool(shuffle)
        self.out_size = tuple(out_size) if out_size is not None else self.recipe.out_size
        Cs = self.images.shape[3]
        self.mean = tuple(mean) if mean is not None else (self.recipe.mean if len(self.recipe.mean) >= Cs else self.recipe.mean * Cs)
        self.std = tuple(std) if std is not None else (self.recipe.std if len(self.recipe.std) >= Cs else self.recipe.std * Cs)
        self.rng = np.random.default_rng(seed)

    def __len__(self) -> int:
        return self.images.shape[0] // self.batch

    def _indices(self) -> Iterator[torch.Tensor]:
        N = self.images.shape[0]
        order = self.rng.permutation(N) if self.shuffle else np.arange(N)
        for i in range(len(self)):
            yield torch.from_numpy(order[i * self.batch:(i + 1) * self.batch].astype(np.int64)).to(self.device)

    def _views(self, idx: torch.Tensor, recipes: Sequence[Recipe], one_launch: bool = True):
        img = self.images.index_select(0, idx)
        msk = self.masks.index_select(0, idx) if self.masks is not None else None
        draws = [draw(r, self.batch, self.rng, self.out_size) for r in recipes]
        seed = int(self.rng.integers(0, 2 ** 62))
        if one_launch or len(draws) == 1:
            return augment_views(img, msk, draws, self.out_size, self.mean, self.std, seed)
        outs = [augment_views(img, msk, d, self.out_size, self.mean, self.std, seed + i) for i, d in enumerate(draws)]
        return (torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]) if msk is not None else None)

    def __iter__(self):
        for idx in self._indices():
            x, y = self._views(idx, (self.recipe,))
            yield x[0], (y[0] if y is not None else None)


class _WeakStrong(ArrayBatches):
    """The unlabelled source of UCC: (x_weak, x_strong, y_weak, y_strong) per batch, UCC/UCC_dataloaders.py:119-143."""
    # Measured (tools/bench_augment_views.py arm b, profiles/augment_views_bench.json): one V = 2 launch takes 1.04x the time of two
    # V = 1 launches (145.0 against 139.6 us, spread 0.4 %), so the two views are launched one after the other.
    ONE_LAUNCH = False

    def __init__(self, images_u8, masks_u8, batch, **kw):
        super().__init__(images_u8, masks_u8, "ucc_weak", batch, **kw)
        self.strong = recipe("ucc_strong")

    def __iter__(self):
        for idx in self._indices():
            x, y = self._views(idx, (self.recipe, self.strong), self.ONE_LAUNCH)
            yield x[0], x[1], (y[0] if y is not None else None), (y[1] if y is not None else None)


class UCCArrayBatches:
    """The two sources UCCTrainer.fit takes, over decoded uint8 arrays: `.train` yields (x, y) under the `ucc_labelled` recipe,
    `.unlabeled` yields (x_weak, x_strong, y_weak, y_strong) -- the weak and the strong view of the same images -- as
    UCCTrainer._unlabeled_inputs requires.  `trainer.fit(src.train, src.unlabeled, val_batches)`."""

    def __init__(self, labelled_images, labelled_masks, unlabelled_images, unlabelled_masks, batch: int, seed: int = 0, **kw):
        self.train = ArrayBatches(labelled_images, labelled_masks, "ucc_labelled", batch, seed=seed, **kw)
        self.unlabeled = _WeakStrong(unlabelled_images, unlabelled_masks, batch, seed=seed + 1, **kw)
