"""Tiled inference without a GPU: the host function `uaps_tile_origins` against `tile_plan`, the mirror formula against numpy's
reflect padding, the named windows, every ValueError / TypeError of the Python surface, the CPU composition against the float64
restatement (tests/tiled_ref.py) over the whole case table, the wiring around a stub network, and the refusals of both entry points
that return before any launch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import tiled_ref as R
from conftest import ROOT

EINVAL, ERANGE = -1, -2


def _origins(n, t, o, cap=128):
    from uaps_amd import _lib
    count, buf = C.c_int(-1), (C.c_int * cap)()
    rc = _lib.lib().uaps_tile_origins(n, t, o, C.byref(count), buf, cap)
    return rc, list(buf[:count.value]) if rc == 0 else None


def test_origins_cover_every_pixel_at_most_three_times():
    from uaps_amd import tile_plan
    for t in (1, 2, 16, 24):
        for o in range(t // 2 + 1):
            for n in range(1, 71):
                rc, got = _origins(n, t, o)
                assert rc == 0
                plan = tile_plan(n, n, t, o)
                assert got == list(plan.ys) == list(plan.xs) == R.origins(n, t, o), (n, t, o)
                assert got == sorted(set(got)) and got[0] == 0
                if n <= t:
                    assert got == [0]
                    continue
                assert got[-1] == n - t
                cover = np.zeros(n, dtype=int)
                for y0 in got:
                    assert 0 <= y0 and y0 + t <= n                      # no tile leaves the image
                    cover[y0:y0 + t] += 1
                assert cover.min() >= 1 and cover.max() <= 3, (n, t, o, cover)
    from uaps_amd import _lib
    L = _lib.lib()
    count = C.c_int(-1)
    assert L.uaps_tile_origins(50, 16, 4, C.byref(count), None, 0) == 0 and count.value == 4        # the count alone
    two = (C.c_int * 3)(-5, -5, -5)
    assert L.uaps_tile_origins(50, 16, 4, C.byref(count), two, 2) == 0 and list(two) == [0, 12, -5]  # never past cap
    assert L.uaps_tile_origins(50, 16, 9, C.byref(count), None, 0) == ERANGE
    assert L.uaps_tile_origins(50, 1, 1, C.byref(count), None, 0) == ERANGE
    for args in ((0, 16, 4), (50, 0, 0), (50, 16, -1)):
        assert L.uaps_tile_origins(*args, C.byref(count), None, 0) == EINVAL
    assert L.uaps_tile_origins(50, 16, 4, None, None, 0) == EINVAL
    assert L.uaps_tile_origins(50, 16, 4, C.byref(count), two, -1) == EINVAL


def test_mirror_is_numpys_reflect_and_defined_beyond_it():
    from uaps_amd.tiled import mirror_index
    for n in range(2, 12):
        for pad in range(0, n):                                         # numpy's reflect accepts any pad for n >= 2
            want = np.pad(np.arange(n), (0, pad), mode="reflect")
            assert [mirror_index(i, n) for i in range(n + pad)] == want.tolist() == [R.mirror(i, n) for i in range(n + pad)]
        many = np.pad(np.arange(n), (0, 3 * n), mode="reflect")
        assert [mirror_index(i, n) for i in range(4 * n)] == many.tolist()
    assert [mirror_index(i, 1) for i in range(20)] == [0] * 20          # n = 1: numpy refuses, the formula does not
    assert [mirror_index(i, 3) for i in range(9)] == [0, 1, 2, 1, 0, 1, 2, 1, 0]


def test_named_windows_and_refusals():
    from uaps_amd import tile_plan, tile_window
    from uaps_amd.tiled import _windows
    assert torch.equal(tile_window(5, "uniform"), torch.ones(5))
    assert tile_window(6, "triangle").tolist() == [1, 2, 3, 3, 2, 1] and tile_window(5, "triangle").tolist() == [1, 2, 3, 2, 1]
    assert tile_window(1, "triangle").tolist() == [1]
    for t in (1, 7, 16):
        for kind in ("uniform", "triangle", "gauss"):
            w = tile_window(t, kind)
            assert w.dtype == torch.float32 and w.shape == (t,)
            assert np.array_equal(w.numpy(), R.window(t, kind).astype(np.float32))
            assert bool((w > 0).all()) and torch.equal(w, w.flip(0))
    g = tile_window(16, "gauss").double()
    k = torch.arange(16, dtype=torch.float64)
    assert float((g - torch.exp(-0.5 * ((k - 7.5) / 2.0) ** 2)).abs().max()) < 1e-7      # sigma = t / 8
    with pytest.raises(ValueError):
        tile_window(8, "hann")
    with pytest.raises(ValueError):
        tile_window(0, "uniform")
    good = torch.ones(8)
    wy, wx = _windows((good, good * 2), (8, 8))
    assert wy.dtype == torch.float32 and torch.equal(wx, good * 2)
    for bad in (torch.zeros(8), -good, good * float("nan"), good * float("inf"),
                torch.tensor([1.0] * 7 + [0.0]), torch.tensor([1.0] * 7 + [float("-inf")])):
        with pytest.raises(ValueError):
            _windows((bad, good), (8, 8))
        with pytest.raises(ValueError):
            _windows((good, bad), (8, 8))
    with pytest.raises(ValueError):
        _windows((torch.ones(7), good), (8, 8))
    for bad in ("hann",):
        with pytest.raises(ValueError):
            _windows(bad, (8, 8))
    for bad in (None, (good,), (good, [1.0] * 8), 3):
        with pytest.raises(TypeError):
            _windows(bad, (8, 8))
    # the plan's refusals
    for args in ((0, 8, 8, 0), (8, 8, 0, 0), (8, 8, 8, 5), (8, 8, 8, -1), (8, 8, (8, 8, 8), 0), (8, 8, 16, (9, 0))):
        with pytest.raises(ValueError):
            tile_plan(*args)
    assert tile_plan(40, 72, (16, 32), (8, 16)).overlap == (8, 16)      # overlap = tile / 2 is legal


class Stub(torch.nn.Module):
    """A seeded 1x1 convolution: a one-head "network" that runs at any size."""

    def __init__(self, cin, classes):
        super().__init__()
        torch.manual_seed(3)
        self.conv = torch.nn.Conv2d(cin, classes, 1)
        self.calls = []

    def forward(self, x):
        self.calls.append(tuple(x.shape))
        return 4.0 * self.conv(x)


def test_python_surface_refusals():
    from uaps_amd import inference, predict_tiled, tile_cut, tile_fold, tile_plan
    x = torch.randn(2, 3, 41, 50)
    plan = tile_plan(41, 50, 16, 4)
    total = 2 * 4 * 4
    z = torch.randn(total, 4, 16, 16)
    with pytest.raises(TypeError):
        tile_cut(x.double(), plan)
    with pytest.raises(TypeError):
        tile_cut(x[0], plan)
    with pytest.raises(ValueError):
        tile_cut(x, tile_plan(40, 50, 16, 4))                           # a plan of another image size
    for g0, g1 in ((-1, 4), (4, 4), (5, 4), (0, total + 1)):
        with pytest.raises(ValueError):
            tile_cut(x, plan, g0, g1)
    dims = (2, 41, 50)
    with pytest.raises(ValueError):
        tile_fold(z, plan, (2, 41))
    with pytest.raises(ValueError):
        tile_fold(z, tile_plan(41, 50, 16, 0), dims)                    # 32 tiles do not fit that plan's 24
    with pytest.raises(ValueError):
        tile_fold(z[:-1], plan, dims)
    with pytest.raises(ValueError):
        tile_fold([z[:5], z[5:12], z[12:]], plan, dims)                 # uneven chunks
    with pytest.raises(ValueError):
        tile_fold([z[k:k + 1] for k in range(total)] + [z[:1]], plan, dims)       # 33 chunks
    with pytest.raises(ValueError):
        tile_fold(z, plan, dims, want=("probs", "logits"))
    with pytest.raises(ValueError):
        tile_fold(z, plan, dims, want=())
    with pytest.raises(ValueError):
        tile_fold(None, plan, dims)                                     # neither logits nor maps
    with pytest.raises(ValueError):
        tile_fold(z, plan, dims, maps=(z[:, 0],) * 3)
    with pytest.raises(ValueError):
        tile_fold(z, plan, dims, maps=([z[:16, 0], z[16:, 0]],))        # maps chunked unlike the logits
    with pytest.raises(ValueError):
        tile_fold(z[:, :1], plan, dims)                                 # one class
    with pytest.raises(ValueError):
        tile_fold(torch.randn(total, 9, 16, 16), plan, dims)
    with pytest.raises(TypeError):
        tile_fold(z.double(), plan, dims)
    with pytest.raises(TypeError):
        tile_fold(z[:, :, :15], plan, dims)
    with pytest.raises(TypeError):
        tile_fold(z, plan, dims, maps=(z,))                             # a map has three dimensions
    with pytest.raises(ValueError):
        tile_fold(z, plan, dims, window=(torch.ones(16), torch.zeros(16)))
    net = Stub(3, 4)
    with pytest.raises(ValueError):
        predict_tiled(net, x, tile=16, overlap=9)
    with pytest.raises(ValueError):
        predict_tiled(net, x, tile=16, overlap=4, batch_tiles=0)
    with pytest.raises(ValueError, match="batch_tiles"):
        predict_tiled(net, torch.randn(1, 3, 64, 64), tile=8, overlap=0, batch_tiles=1)     # 64 chunks
    with pytest.raises(ValueError):
        predict_tiled(net, x, tile=16, overlap=4, uncertainty=True)     # a one-head model
    with pytest.raises(TypeError):
        predict_tiled(net, x.double(), tile=16)
    from uaps_amd import UNet
    with pytest.raises(ValueError, match="multiple"):
        predict_tiled(UNet(3, 4), x, tile=24, overlap=4)
    batches = [(x, torch.zeros(2, 41, 50, dtype=torch.int64))]
    with pytest.raises(ValueError):
        inference.evaluate(net, batches, tta=True, tiled=True)
    with pytest.raises(ValueError):
        inference.predict_instances(net, x, tta=True, tiled={"tile": 16})
    with pytest.raises(TypeError):
        inference.evaluate(net, batches, tiled=16)


def test_cpu_cut_is_exact():
    from uaps_amd import tile_cut, tile_plan
    gen = torch.Generator().manual_seed(7)
    for case in R.CASES:
        x = torch.randn(case.B, 3, case.H, case.W, generator=gen)
        plan = tile_plan(case.H, case.W, case.tile, case.overlap)
        want = R.cut(x, case.tile, case.overlap)
        got = tile_cut(x, plan)
        assert got.shape == (R.n_tiles(case), 3) + case.tile and torch.equal(got, want)
        assert torch.equal(tile_cut(x, plan, 1 if got.shape[0] > 1 else 0, got.shape[0]), want[1 if got.shape[0] > 1 else 0:])
    x = torch.randn(2, 3, 16, 24, generator=gen)
    assert torch.equal(tile_cut(x, tile_plan(16, 24, (16, 24), (8, 12))), x)      # tile = image
    # the mirror padding is numpy's reflect padding
    small = torch.randn(1, 2, 5, 7, generator=gen)
    padded = np.pad(small.numpy(), ((0, 0), (0, 0), (0, 4), (0, 6)), mode="reflect")
    assert np.array_equal(tile_cut(small, tile_plan(5, 7, (9, 13), 0)).numpy(), padded)


@pytest.mark.parametrize("name,kind", R.CASE_WINDOWS, ids=[f"{n}-{k}" for n, k in R.CASE_WINDOWS])
def test_cpu_fold_against_float64(name, kind):
    from uaps_amd import tile_fold, tile_plan
    case, z, ref = R.reference(name, kind)
    plan = tile_plan(case.H, case.W, case.tile, case.overlap)
    dims = (case.B, case.H, case.W)
    res = tile_fold(z, plan, dims, kind)
    assert res.probs.dtype == torch.float32 and res.mask.dtype == torch.int64 and res.maps == ()
    e_p, e_c = R.check_result(res, ref, name)
    print(f"{name} {kind}: probs err {e_p:.3e}, conf err {e_c:.3e}, bar {R.TAU:.2e}")
    chunks = tile_fold(R.chunked(z), plan, dims, kind)
    assert torch.equal(chunks.probs, res.probs) and torch.equal(chunks.mask, res.mask) and torch.equal(chunks.conf, res.conf)
    only = tile_fold(z, plan, dims, kind, want=("mask",))
    assert only.probs is None and only.conf is None and torch.equal(only.mask, res.mask)
    if name == "exact-32x48":                   # no overlap: the result IS the tiles' softmax, in image-major numbering
        sm = torch.softmax(z, dim=1).view(case.B, 2, 3, case.C, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(case.B, case.C, 32, 48)
        assert float((res.probs - sm).abs().max()) <= 2.0 ** -23
    # a window given as tensors is the named one
    wy, wx = (torch.from_numpy(R.window(t, kind).astype(np.float32)) for t in case.tile)
    assert torch.equal(tile_fold(z, plan, dims, (wy, wx)).probs, res.probs)


def test_cpu_maps_blend_back_to_a_function_of_the_image_coordinates():
    from uaps_amd import tile_cut, tile_fold, tile_plan
    B, H, W = 2, 41, 50
    plan = tile_plan(H, W, 16, 4)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    f = torch.stack([(yy * 64 + xx) / 4096, (xx * 64 + yy) / 4096 + 0.25])                  # exact in fp32, below 1, one per image
    g = 1.0 - f
    mf, mg = tile_cut(f[:, None], plan)[:, 0], tile_cut(g[:, None], plan)[:, 0]
    res = tile_fold(None, plan, (B, H, W), "triangle", maps=(mf, mg))
    assert res.probs is None and res.mask is None and res.conf is None and len(res.maps) == 2
    assert float((res.maps[0] - f).abs().max()) <= R.TAU and float((res.maps[1] - g).abs().max()) <= R.TAU
    z = torch.randn(mf.shape[0], 3, 16, 16, generator=torch.Generator().manual_seed(1))
    both = tile_fold(R.chunked(z), plan, (B, H, W), "gauss", maps=(R.chunked(mf),), want=("mask",))
    assert both.mask.shape == (B, H, W) and float((both.maps[0] - f).abs().max()) <= R.TAU
    ref, rmaps = R.fold(z, (B, H, W), (16, 16), (4, 4), R.window(16, "gauss"), R.window(16, "gauss"), maps=(mf,))
    R.check_mask(both.mask, ref)
    assert float((both.maps[0].double() - rmaps[0]).abs().max()) <= R.TAU


def _host_confusion(scored, labels):
    """The metrics kernel needs the GPU: count on the host what evaluate hands it."""
    B, Cc = scored.shape[:2]
    return torch.stack([torch.bincount(labels[b].flatten() * Cc + scored[b].argmax(0).flatten(), minlength=Cc * Cc).view(Cc, Cc)
                        for b in range(B)])


def test_predict_tiled_around_a_stub(monkeypatch):
    from uaps_amd import inference, metrics, predict_tiled, tile_cut, tile_fold, tile_plan
    x = torch.randn(2, 3, 41, 50, generator=torch.Generator().manual_seed(5))
    net = Stub(3, 4)
    plan = tile_plan(41, 50, 16, 4)
    net.train()
    res = predict_tiled(net, x, tile=16, overlap=4)
    assert not net.training and net.calls == [(32, 3, 16, 16)]                     # one forward of every tile
    with torch.no_grad():
        want = tile_fold(net(tile_cut(x, plan)), plan, (2, 41, 50))
        whole = torch.softmax(net(x).double(), dim=1)
    assert torch.equal(res.probs, want.probs) and torch.equal(res.mask, want.mask) and torch.equal(res.conf, want.conf)
    assert not res.probs.requires_grad
    # a 1x1 convolution sees no context: every tile's softmax is the whole image's, and so is their weighted mean
    assert float((res.probs.double() - whole).abs().max()) <= 1e-5             # the fp32 forwards of a tile and of the image differ in rounding
    net.calls.clear()
    chunked = predict_tiled(net, x, tile=16, overlap=4, batch_tiles=5, window="gauss", want=("probs",))
    assert [c[0] for c in net.calls] == [5] * 6 + [2] and chunked.mask is None
    assert float((chunked.probs.double() - whole).abs().max()) <= 1e-5
    y = whole.argmax(1)
    monkeypatch.setattr(metrics, "seg_confusion_per_image", _host_confusion)
    out = inference.evaluate(net, [(x, y), (x.flip(3), y.flip(2))], tiled={"tile": 16, "overlap": 4})
    assert out["images"] == 4 and out["Accuracy(%)"] > 99.0
    auto = predict_tiled(net, x, tile=16, overlap=4, uncertainty="auto", want=("mask",))    # one head: no map
    assert auto.maps == () and torch.equal(auto.mask, res.mask)


def test_evaluate_defaults_do_not_touch_the_tiled_path(monkeypatch):
    from uaps_amd import inference, metrics, tiled
    monkeypatch.setattr(metrics, "seg_confusion_per_image", _host_confusion)
    monkeypatch.setattr(tiled, "predict_tiled", lambda *a, **k: pytest.fail("predict_tiled called without tiled"))
    net = Stub(3, 4)
    gen = torch.Generator().manual_seed(2)
    batches = [(torch.randn(2, 3, 16, 16, generator=gen), torch.randint(0, 4, (2, 16, 16), generator=gen))]
    assert inference.evaluate(net, batches) == inference.evaluate(net, batches, tiled=None) == inference.evaluate(net, batches, tiled=False)


def test_c_abi_symbols_struct_sizes_and_refusals_before_any_launch(tmp_path):
    from uaps_amd import _lib
    L = _lib.lib()
    assert L.uaps_abi_version() == 3
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "uaps_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(uaps_tile_cut_call), sizeof(uaps_tile_fold_call),\n'
                   '    offsetof(uaps_tile_cut_call, x), offsetof(uaps_tile_fold_call, logits), offsetof(uaps_tile_fold_call, maps),\n'
                   '    offsetof(uaps_tile_fold_call, map_out), UAPS_TILE_MAX_CHUNKS, UAPS_TILE_MAX_MAPS); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(_lib.TileCutCall), C.sizeof(_lib.TileFoldCall), _lib.TileCutCall.x.offset,
                                     _lib.TileFoldCall.logits.offset, _lib.TileFoldCall.maps.offset, _lib.TileFoldCall.map_out.offset,
                                     _lib.TILE_MAX_CHUNKS, _lib.TILE_MAX_MAPS] and _lib.TILE_MAX_CHUNKS == 32 and _lib.TILE_MAX_MAPS == 2
    assert L.uaps_tile_cut(None) == EINVAL and L.uaps_tile_fold(None) == EINVAL
    # dummy non-NULL pointers: every one of these returns before anything is launched or read
    P = 4096
    dims = {"B": 2, "Cin": 3, "H": 41, "W": 50}
    cfull = C.sizeof(_lib.TileCutCall)
    cut_cases = [({"x": None}, EINVAL), ({"out": None}, EINVAL), ({"B": 0}, EINVAL), ({"Cin": -1}, EINVAL), ({"H": 0}, EINVAL),
                 ({"W": 0}, EINVAL), ({"th": 0}, EINVAL), ({"tw": -16}, EINVAL), ({"oy": -1}, EINVAL), ({"ox": -1}, EINVAL),
                 ({"struct_size": cfull - 8}, EINVAL), ({"struct_size": 4}, EINVAL), ({"g0": -1}, EINVAL), ({"g0": 5, "g1": 5}, EINVAL),
                 ({"g0": 6, "g1": 5}, EINVAL), ({"g1": 33}, EINVAL), ({"oy": 9}, ERANGE), ({"ox": 9}, ERANGE),
                 ({"B": 64, "Cin": 8, "H": 1024, "W": 1024}, ERANGE),                                 # x at 2 GiB
                 ({"th": 8192, "tw": 8192, "H": 10000, "W": 10000, "B": 1, "g1": 4, "oy": 0, "ox": 0}, ERANGE)]   # the chunk beyond 2 GiB
    for kw, want in cut_cases:
        assert R.raw_cut(P, P, (16, 16), (4, 4), 0, 32, over={**dims, **kw}) == want, kw
    ffull = C.sizeof(_lib.TileFoldCall)
    chunks = [P] * 11                                                   # 32 tiles in chunks of 3

    def fold(over, **kw):
        args = dict(probs=P, mask=P, conf=P, per=3, n_classes=4)
        args.update(kw)
        return R.raw_fold(chunks, (2, 41, 50), (16, 16), (4, 4), P, P, over=over, **args)
    fold_cases = [({"wy": None}, EINVAL), ({"wx": None}, EINVAL), ({"B": 0}, EINVAL), ({"H": 0}, EINVAL), ({"W": -3}, EINVAL),
                  ({"th": 0}, EINVAL), ({"tw": 0}, EINVAL), ({"oy": -1}, EINVAL), ({"C": -1}, EINVAL), ({"C": 0}, EINVAL),
                  ({"n_maps": -1}, EINVAL), ({"n_chunks": 0}, EINVAL), ({"tiles_per_chunk": 0}, EINVAL),
                  ({"struct_size": ffull - 8}, EINVAL), ({"struct_size": 8}, EINVAL),
                  ({"logits0": None}, EINVAL), ({"logits10": None}, EINVAL),                          # a chunk pointer missing below the count
                  ({"n_chunks": 12}, EINVAL), ({"n_chunks": 10}, EINVAL), ({"tiles_per_chunk": 2}, EINVAL),
                  ({"n_maps": 1}, EINVAL),                                                            # a map without its chunks
                  ({"oy": 9}, ERANGE), ({"ox": 9}, ERANGE), ({"C": 1}, ERANGE), ({"C": 9}, ERANGE), ({"n_maps": 3}, ERANGE),
                  ({"n_chunks": 33, "tiles_per_chunk": 1}, ERANGE),
                  ({"B": 64, "C": 8, "H": 1024, "W": 1024}, ERANGE),                                  # probs at 2 GiB
                  ({"B": 256, "C": 2, "H": 1024, "W": 1024}, ERANGE),                                 # the mask at 2 GiB
                  ({"th": 8192, "tw": 8192, "H": 20000, "W": 20000, "B": 1, "oy": 0, "ox": 0, "tiles_per_chunk": 9, "n_chunks": 1,
                    "probs": None, "mask": None}, ERANGE)]                                            # a chunk of logits beyond 2 GiB
    for kw, want in fold_cases:
        assert fold(kw) == want, kw
    assert fold(None, probs=None, mask=None, conf=None) == EINVAL                                   # no output at all
    maps = [[P] * 11]
    assert fold({"map_out0": None}, maps=maps, map_out=[P]) == EINVAL
    assert fold({"maps4": None}, maps=maps, map_out=[P]) == EINVAL
    assert fold({"C": 0}, maps=maps, map_out=[P]) == EINVAL                                         # class outputs without classes
