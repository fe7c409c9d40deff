"""Tiled (sliding-window) inference on the GPU (csrc/tiled.hip): the cut kernel against the numpy-indexed restatement, the fold kernel
over the case table of tests/tiled_ref.py against the float64 scatter form (every window, both store forms, chunked logits, subsets of
the outputs, two runs), blended maps, every error return of the C ABI, a later header's struct, and the wiring around the real
network.  The bars and their derivation: tests/tiled_ref.py; the measured errors: profiles/tiled_forms_tau.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import tiled_ref as R

pytestmark = pytest.mark.gpu
DEV = R.DEV
EINVAL, ERANGE = -1, -2
SENTINEL = -12345.0


def _plan(case):
    from uaps_amd import tile_plan
    return tile_plan(case.H, case.W, case.tile, case.overlap)


def _dev_windows(case, kind):
    return tuple(torch.from_numpy(R.window(t, kind).astype(np.float32)).to(DEV) for t in case.tile)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_cut_is_exact(name):
    from uaps_amd import tile_cut
    case = next(c for c in R.CASES if c.name == name)
    x_cpu = torch.randn(case.B, 3, case.H, case.W, generator=torch.Generator().manual_seed(7))
    x, plan = x_cpu.to(DEV), _plan(case)
    want = R.cut(x_cpu, case.tile, case.overlap)
    got = tile_cut(x, plan)
    assert got.shape == want.shape and torch.equal(got.cpu(), want)
    total = want.shape[0]
    if total > 1:                               # one chunk of the tiles: a launch writes [g0, g1) alone
        buf = torch.full((total + 1, 3) + case.tile, SENTINEL, device=DEV)
        assert R.raw_cut(x, buf[1:], case.tile, case.overlap, 1, total - 1 if total > 2 else total) == 0
        n = (total - 2) if total > 2 else (total - 1)
        assert torch.equal(buf[1:1 + n].cpu(), want[1:1 + n])
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[1 + n:] == SENTINEL).all())


def test_cut_with_tile_equal_to_image_is_the_image():
    from uaps_amd import tile_cut, tile_plan
    x = torch.randn(2, 3, 16, 24, device=DEV)
    assert torch.equal(tile_cut(x, tile_plan(16, 24, (16, 24), (8, 12))), x)


@pytest.mark.parametrize("name,kind", R.CASE_WINDOWS, ids=[f"{n}-{k}" for n, k in R.CASE_WINDOWS])
def test_fold_against_float64(name, kind):
    from uaps_amd import tile_fold
    case, z_cpu, ref = R.reference(name, kind)
    z, plan, dims = z_cpu.to(DEV), _plan(case), (case.B, case.H, case.W)
    res = tile_fold(z, plan, dims, kind)
    e_p, e_c = R.check_result(res, ref, name)
    print(f"{name} {kind}: probs err {e_p:.3e}, conf err {e_c:.3e}, bar {R.TAU:.2e}")
    # chunked logits (a short last chunk, chunk boundaries inside an image): the same bits
    ch = tile_fold(R.chunked(z), plan, dims, kind)
    assert torch.equal(ch.probs, res.probs) and torch.equal(ch.mask, res.mask) and torch.equal(ch.conf, res.conf)
    # a subset of the outputs: the same bits
    only_mask, only_probs = tile_fold(z, plan, dims, kind, want=("mask",)), tile_fold(z, plan, dims, kind, want=("probs",))
    only_conf = tile_fold(z, plan, dims, kind, want=("conf",))
    assert only_mask.probs is None and only_mask.conf is None and torch.equal(only_mask.mask, res.mask)
    assert only_probs.mask is None and torch.equal(only_probs.probs, res.probs) and torch.equal(only_conf.conf, res.conf)
    # two runs: the same bits
    again = tile_fold(z, plan, dims, kind)
    assert torch.equal(again.probs, res.probs) and torch.equal(again.mask, res.mask) and torch.equal(again.conf, res.conf)
    # outputs at storage offset 1 (no 16-byte alignment: the one-pixel form), sentinels on both sides: the same arithmetic per pixel
    n = case.B * case.H * case.W
    pb = torch.full((n * case.C + 2,), SENTINEL, device=DEV)
    mb = torch.full((n + 2,), -7, dtype=torch.int64, device=DEV)
    cb = torch.full((n + 2,), SENTINEL, device=DEV)
    wy, wx = _dev_windows(case, kind)
    assert R.raw_fold([z], dims, case.tile, case.overlap, wy, wx, pb[1:], mb[1:], cb[1:]) == 0
    p1, m1, c1 = pb[1:-1].view(case.B, case.C, case.H, case.W), mb[1:-1].view(dims), cb[1:-1].view(dims)
    from uaps_amd.tiled import TiledResult
    R.check_result(TiledResult(p1, m1, c1, ()), ref, name)
    assert torch.equal(p1, res.probs) and torch.equal(m1, res.mask) and torch.equal(c1, res.conf)
    assert float(pb[0]) == SENTINEL and float(pb[-1]) == SENTINEL and int(mb[0]) == -7 and int(mb[-1]) == -7
    assert float(cb[0]) == SENTINEL and float(cb[-1]) == SENTINEL
    # aligned outputs through the raw call, sentinels behind them
    pa = torch.full((n * case.C + 4,), SENTINEL, device=DEV)
    assert R.raw_fold(R.chunked(z), dims, case.tile, case.overlap, wy, wx, pa) == 0
    assert torch.equal(pa[:-4].view_as(res.probs), res.probs) and bool((pa[-4:] == SENTINEL).all())


def test_no_overlap_is_the_tiles_softmax():
    from uaps_amd import tile_fold
    case, z_cpu, _ = R.reference("exact-32x48", "uniform")
    res = tile_fold(z_cpu.to(DEV), _plan(case), (case.B, case.H, case.W), "uniform", want=("probs",))
    sm = torch.softmax(z_cpu.double(), dim=1).view(case.B, 2, 3, case.C, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(case.B, case.C, 32, 48)
    assert float((res.probs.cpu().double() - sm).abs().max()) <= R.TAU


@pytest.mark.parametrize("shape,tile,overlap", (((2, 41, 50), (16, 16), (4, 4)), ((1, 40, 72), (16, 32), (8, 16)), ((2, 5, 7), (16, 16), (0, 0))),
                         ids=("clamp-41x50", "half-40x72", "small-5x7"))
def test_maps_blend_back_to_a_function_of_the_image_coordinates(shape, tile, overlap):
    """A per-tile map equal to a function of the image coordinates blends back to that function: a wrong origin cannot."""
    from uaps_amd import tile_cut, tile_fold, tile_plan
    B, H, W = shape
    plan = tile_plan(H, W, tile, overlap)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    f = torch.stack([(yy * 128 + xx + b) / 8192 for b in range(B)]).to(DEV)       # exact in fp32, below 1, another per image
    g = 1.0 - f
    mf, mg = tile_cut(f[:, None], plan)[:, 0].contiguous(), tile_cut(g[:, None], plan)[:, 0].contiguous()
    for kind in ("uniform", "triangle", "gauss"):
        res = tile_fold(None, plan, shape, kind, maps=(mf, mg))                   # maps alone: no logits
        assert res.probs is None and res.mask is None and res.conf is None and len(res.maps) == 2
        e = max(float((res.maps[0] - f).abs().max()), float((res.maps[1] - g).abs().max()))
        print(f"{shape} {kind}: map err {e:.3e}, bar {R.TAU:.2e}")
        assert e <= R.TAU
    # beside logits, chunked, one map: the logits' outputs keep their bits, the map is the float64 blend
    z_cpu = torch.randn(mf.shape[0], 3, *tile, generator=torch.Generator().manual_seed(1)) * 2
    z = z_cpu.to(DEV)
    plain = tile_fold(z, plan, shape, "triangle")
    both = tile_fold(R.chunked(z), plan, shape, "triangle", maps=(R.chunked(mf),))
    assert torch.equal(both.probs, plain.probs) and torch.equal(both.mask, plain.mask) and torch.equal(both.conf, plain.conf)
    _, rmaps = R.fold(None, shape, tile, overlap, R.window(tile[0], "triangle"), R.window(tile[1], "triangle"), maps=(mf.cpu(),))
    assert float((both.maps[0].cpu().double() - rmaps[0]).abs().max()) <= R.TAU
    assert torch.equal(both.maps[0], tile_fold(None, plan, shape, "triangle", maps=(mf,)).maps[0])


def test_every_error_return_writes_nothing():
    from uaps_amd import _lib
    L = _lib.lib()
    B, Cc, H, W, tile, overlap = 2, 4, 41, 52, (16, 16), (4, 4)
    total = 2 * 4 * 4
    z = torch.randn(total, Cc, 16, 16, device=DEV)
    chunks = R.chunked(z)                                               # 11 chunks of 3
    mp = R.chunked(z[:, 0].contiguous())
    wy = wx = torch.ones(16, device=DEV)
    probs = torch.full((B, Cc, H, W), SENTINEL, device=DEV)
    mask = torch.full((B, H, W), -7, dtype=torch.int64, device=DEV)
    conf = torch.full((B, H, W), SENTINEL, device=DEV)
    mo = torch.full((B, H, W), SENTINEL, device=DEV)
    full = C.sizeof(_lib.TileFoldCall)

    def fold(over, **kw):
        args = dict(probs=probs, mask=mask, conf=conf, maps=[mp], map_out=[mo])
        args.update(kw)
        return R.raw_fold(chunks, (B, H, W), tile, overlap, wy, wx, over=over, **args)
    assert L.uaps_tile_fold(None) == EINVAL
    assert fold(None, probs=None, mask=None, conf=None, maps=[], map_out=[]) == EINVAL                # no output at all
    assert fold(None, probs=None, mask=None, conf=None) == EINVAL                                     # classes without a class output
    cases = [({"wy": None}, EINVAL), ({"wx": None}, EINVAL), ({"logits0": None}, EINVAL), ({"logits10": None}, EINVAL),
             ({"maps0": None}, EINVAL), ({"maps10": None}, EINVAL), ({"map_out0": None}, EINVAL),
             ({"B": 0}, EINVAL), ({"H": -1}, EINVAL), ({"W": 0}, EINVAL), ({"th": 0}, EINVAL), ({"tw": 0}, EINVAL), ({"oy": -1}, EINVAL),
             ({"ox": -4}, EINVAL), ({"C": -2}, EINVAL), ({"C": 0}, EINVAL), ({"n_maps": -1}, EINVAL), ({"n_chunks": 0}, EINVAL),
             ({"tiles_per_chunk": 0}, EINVAL), ({"n_chunks": 10}, EINVAL), ({"n_chunks": 12}, EINVAL), ({"tiles_per_chunk": 4}, EINVAL),
             ({"struct_size": full - 8}, EINVAL), ({"struct_size": 8}, EINVAL),
             ({"oy": 9}, ERANGE), ({"ox": 9}, ERANGE), ({"C": 1}, ERANGE), ({"C": 9}, ERANGE), ({"n_maps": 3}, ERANGE),
             ({"n_chunks": 33, "tiles_per_chunk": 1}, ERANGE),
             ({"B": 64, "C": 8, "H": 1024, "W": 1024}, ERANGE),                                       # probs at 2 GiB
             ({"B": 256, "C": 2, "H": 1024, "W": 1024}, ERANGE)]                                      # the mask at 2 GiB
    for kw, want in cases:
        assert fold(kw) == want, kw
    # a chunk of logits beyond 2 GiB, with conf (1.6 GB by dimensions) the only output
    big = {"th": 8192, "tw": 8192, "H": 20000, "W": 20000, "B": 1, "oy": 0, "ox": 0, "tiles_per_chunk": 9, "n_chunks": 1}
    assert fold(big, probs=None, mask=None, maps=[], map_out=[]) == ERANGE
    x = torch.randn(B, 3, H, W, device=DEV)
    out = torch.full((total, 3, 16, 16), SENTINEL, device=DEV)
    assert L.uaps_tile_cut(None) == EINVAL
    cfull = C.sizeof(_lib.TileCutCall)
    ccases = [({"x": None}, EINVAL), ({"out": None}, EINVAL), ({"B": 0}, EINVAL), ({"Cin": 0}, EINVAL), ({"H": 0}, EINVAL), ({"W": -1}, EINVAL),
              ({"th": 0}, EINVAL), ({"tw": 0}, EINVAL), ({"oy": -1}, EINVAL), ({"ox": -1}, EINVAL), ({"g0": -1}, EINVAL),
              ({"g0": 4, "g1": 4}, EINVAL), ({"g0": 5, "g1": 4}, EINVAL), ({"g1": total + 1}, EINVAL),
              ({"struct_size": cfull - 8}, EINVAL), ({"struct_size": 4}, EINVAL), ({"oy": 9}, ERANGE), ({"ox": 9}, ERANGE),
              ({"B": 64, "Cin": 8, "H": 1024, "W": 1024}, ERANGE),
              ({"th": 8192, "tw": 8192, "H": 10000, "W": 10000, "B": 1, "g1": 4, "oy": 0, "ox": 0}, ERANGE)]
    for kw, want in ccases:
        assert R.raw_cut(x, out, tile, overlap, 0, total, over=kw) == want, kw
    torch.cuda.synchronize()
    assert bool((probs == SENTINEL).all()) and bool((mask == -7).all()) and bool((conf == SENTINEL).all())
    assert bool((mo == SENTINEL).all()) and bool((out == SENTINEL).all())


def test_a_later_headers_struct_is_accepted():
    """A larger struct_size: this version's fields are read, what follows is not; the Python surface's bits come back."""
    from uaps_amd import _lib, tile_cut, tile_fold
    case, z_cpu, _ = R.reference("clamp-41x50", "triangle")
    z, plan, dims = z_cpu.to(DEV), _plan(case), (case.B, case.H, case.W)
    want = tile_fold(z, plan, dims, "triangle")

    class Later(C.Structure):
        _fields_ = [("base", _lib.TileFoldCall), ("appended", C.c_double * 4)]
    probs, mask, conf = torch.empty_like(want.probs), torch.empty_like(want.mask), torch.empty_like(want.conf)
    wy, wx = _dev_windows(case, "triangle")
    assert R.raw_fold([z], dims, case.tile, case.overlap, wy, wx, probs, mask, conf, struct=Later()) == 0
    assert torch.equal(probs, want.probs) and torch.equal(mask, want.mask) and torch.equal(conf, want.conf)

    class LaterCut(C.Structure):
        _fields_ = [("base", _lib.TileCutCall), ("appended", C.c_double * 4)]
    x = torch.randn(case.B, 3, case.H, case.W, device=DEV)
    out = torch.empty(z.shape[0], 3, *case.tile, device=DEV)
    assert R.raw_cut(x, out, case.tile, case.overlap, 0, z.shape[0], struct=LaterCut()) == 0
    assert torch.equal(out, tile_cut(x, plan))


@pytest.fixture(scope="module")
def net():
    import uaps_amd
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet_uaps", 3, 4)
    x = torch.randn(2, 3, 80, 112, generator=torch.Generator().manual_seed(9)).to(DEV)
    return model.eval(), x


def test_wiring_on_the_real_network(net):
    from uaps_amd import predict_tiled, tile_cut, tile_fold, tile_plan
    model, x = net
    plan = tile_plan(80, 112, 64, 16)
    assert plan.ys == (0, 16) and plan.xs == (0, 48)                    # 2 x 2 tiles per image, one of each pair clamped
    with torch.no_grad():
        res = predict_tiled(model, x, tile=64, overlap=16)
        tiles = tile_cut(x, plan)
        z = model.forward_main(tiles)
        want = tile_fold(z, plan, (2, 80, 112))
        assert torch.equal(res.probs, want.probs) and torch.equal(res.mask, want.mask) and torch.equal(res.conf, want.conf)
        assert res.probs.shape == (2, 4, 80, 112) and res.mask.shape == (2, 80, 112) and res.maps == ()
        # a float64 composition behind the network
        ref, _ = R.fold(z.cpu(), (2, 80, 112), (64, 64), (16, 16), R.window(64, "triangle"), R.window(64, "triangle"))
        R.check_mask(res.mask, ref)
        assert float((res.probs.cpu().double() - ref).abs().max()) <= R.TAU
        assert float((res.probs.sum(1) - 1).abs().max()) <= R.TAU
        unc = predict_tiled(model, x, tile=64, overlap=16, uncertainty=True, want=("mask", "conf"))
        assert unc.probs is None and len(unc.maps) == 1 and unc.maps[0].shape == (2, 80, 112)
        assert bool(torch.isfinite(unc.maps[0]).all())
        parts = predict_tiled(model, x, tile=64, overlap=16, batch_tiles=3, want=("mask",))         # 3 + 3 + 2 tiles
        assert parts.mask.shape == (2, 80, 112)


def test_evaluate_and_instances_with_tiles(net):
    from uaps_amd import inference
    from uaps_amd.instances import InstanceResult
    model, x = net
    y = torch.randint(0, 4, (2, 80, 112), generator=torch.Generator().manual_seed(4)).to(DEV)
    batches = [(x, y), (x.flip(2), y)]
    out = inference.evaluate(model, batches, tiled={"tile": 64, "overlap": 16})
    assert out["images"] == 4 and all(0.0 <= out[k] <= 100.0 for k in ("mIoU(%)", "mDice(%)", "Accuracy(%)"))
    assert inference.evaluate(model, [(x[:, :, :64, :64].contiguous(), y[:, :64, :64].contiguous())], tiled=True)["images"] == 2
    r = inference.predict_instances(model, x, tiled={"tile": 64, "overlap": 16})
    assert isinstance(r, InstanceResult) and r.labels.shape == (2, 80, 112)
    with pytest.raises(ValueError):
        inference.predict_instances(model, x, tta=True, tiled={"tile": 64, "overlap": 16})
    with pytest.raises(ValueError):
        inference.evaluate(model, batches, tta=True, tiled=True)
