"""Test-time augmentation on the GPU (csrc/tta.hip): the fold kernel over the case table of tests/tta_ref.py against float64 (every
class-count / scale-count / vector-form / degenerate-size branch), the views kernel, every error return of the C ABI, and the wiring
around the real network.  The bars and their derivation: tests/tta_ref.py; the measured errors: profiles/tta_forms_tau.txt."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import tta_ref as R

pytestmark = pytest.mark.gpu
DEV = R.DEV
raw_fold = R.raw_fold
EINVAL, ERANGE = -1, -2
SENTINEL = -12345.0


@pytest.mark.parametrize("flip", (True, False), ids=("flip", "plain"))
@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_fold_against_float64(name, flip):
    from uaps_amd import tta_fold
    case, zs_cpu, ref = R.reference(name, flip)
    zs = [z.to(DEV) for z in zs_cpu]
    size, views = (case.H, case.W), len(zs) * (2 if flip else 1)
    res = tta_fold(zs, size, flip)
    e_sum = float((res.probs.cpu().double() - ref).abs().max())
    e_conf = float((res.conf.cpu().double() - ref.max(dim=1).values / views).abs().max())
    print(f"{name} flip={flip}: probs_sum err {e_sum:.3e}, conf err {e_conf:.3e}, bar {R.TAU_SUM:.1e}")
    assert e_sum <= R.TAU_SUM and e_conf <= R.TAU_SUM
    R.check_mask(res.mask, ref)
    assert torch.equal(res.mask, res.probs.argmax(dim=1))                          # lowest index on ties, as torch
    assert float((res.conf - res.probs.max(dim=1).values / views).abs().max()) <= 2e-7      # one rounding of a value <= 1
    # a subset of the outputs: the same bits
    only_mask, only_probs = tta_fold(zs, size, flip, want=("mask",)), tta_fold(zs, size, flip, want=("probs",))
    assert only_mask.probs is None and only_mask.conf is None and torch.equal(only_mask.mask, res.mask)
    assert only_probs.mask is None and torch.equal(only_probs.probs, res.probs)
    # two runs: the same bits
    again = tta_fold(zs, size, flip)
    assert torch.equal(again.probs, res.probs) and torch.equal(again.mask, res.mask) and torch.equal(again.conf, res.conf)
    # outputs at storage offset 1 (no 16-byte alignment: the one-pixel form): the same values to the bar
    n = case.B * case.H * case.W
    pb = torch.full((n * case.C + 2,), SENTINEL, device=DEV)
    mb = torch.full((n + 2,), -7, dtype=torch.int64, device=DEV)
    cb = torch.full((n + 2,), SENTINEL, device=DEV)
    assert raw_fold(zs, (case.B, case.H, case.W), flip, pb[1:], mb[1:], cb[1:]) == 0
    p1 = pb[1:-1].view(case.B, case.C, case.H, case.W)
    assert float((p1.cpu().double() - ref).abs().max()) <= R.TAU_SUM
    assert float((p1 - res.probs).abs().max()) <= R.TAU_SUM and float((cb[1:-1].view_as(res.conf) - res.conf).abs().max()) <= R.TAU_SUM
    R.check_mask(mb[1:-1].view_as(res.mask), ref)
    assert float(pb[0]) == SENTINEL and float(pb[-1]) == SENTINEL and int(mb[0]) == -7 and int(mb[-1]) == -7
    assert float(cb[0]) == SENTINEL and float(cb[-1]) == SENTINEL


@pytest.mark.parametrize("shape", R.VIEW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_views(shape):
    from uaps_amd import tta_views
    B, Cin, H, W = shape
    x_cpu = torch.randn(*shape, generator=torch.Generator().manual_seed(5))
    x = x_cpu.to(DEV)
    same = tta_views(x, (H, W))
    assert same.shape == (2 * B, Cin, H, W)
    assert torch.equal(same[:B], x) and torch.equal(same[B:], x.flip(3))
    for size in R.VIEW_SIZES:
        v = tta_views(x, size)
        err = float((v.cpu().double() - R.views(x_cpu, size)).abs().max())
        print(f"{shape} -> {size}: err {err:.3e}, bar {R.TAU_VIEWS:.1e}")
        assert v.shape == (2 * B, Cin) + size and err <= R.TAU_VIEWS
        assert torch.equal(v[B:], v[:B].flip(3))
        assert torch.equal(tta_views(x, size, flip=False), v[:B])


def raw_views(x, out, h, w, flip, over=None):
    from uaps_amd import _lib
    call = _lib.TTAViewsCall(C.sizeof(_lib.TTAViewsCall), x.shape[0], x.shape[1], x.shape[2], x.shape[3], h, w,
                             int(flip), x.data_ptr(), out.data_ptr(), _lib.current_stream(x.device))
    for k, v in (over or {}).items():
        setattr(call, k, v)
    return _lib.lib().uaps_tta_views(C.byref(call))


def test_views_without_flip_write_b_images():
    B, Cin, H, W, h, w = 2, 3, 32, 48, 24, 36
    x = torch.randn(B, Cin, H, W, device=DEV)
    buf = torch.full((2 * B, Cin, h, w), SENTINEL, device=DEV)
    assert raw_views(x, buf, h, w, 0) == 0
    assert bool((buf[B:] == SENTINEL).all()) and not bool((buf[:B] == SENTINEL).any())
    from uaps_amd import tta_views
    assert torch.equal(buf[:B], tta_views(x, (h, w), flip=False)) and torch.equal(buf[:B], tta_views(x, (h, w))[:B])


def test_every_error_return_writes_nothing():
    from uaps_amd import _lib
    L = _lib.lib()
    B, Cc, H, W = 2, 4, 16, 24
    zs = [torch.randn(2 * B, Cc, h, w, device=DEV) for h, w in ((8, 12), (16, 24))]
    probs = torch.full((B, Cc, H, W), SENTINEL, device=DEV)
    mask = torch.full((B, H, W), -7, dtype=torch.int64, device=DEV)
    conf = torch.full((B, H, W), SENTINEL, device=DEV)
    full = C.sizeof(_lib.TTAFoldCall)
    assert L.uaps_tta_fold(None) == EINVAL
    assert raw_fold(zs, (B, H, W), True) == EINVAL                                                        # all three outputs NULL
    cases = [({"logits0": None}, EINVAL), ({"logits1": None}, EINVAL), ({"B": 0}, EINVAL), ({"H": -1}, EINVAL), ({"W": 0}, EINVAL),
             ({"C": 0}, EINVAL), ({"h1": 0}, EINVAL), ({"w0": -2}, EINVAL), ({"struct_size": full - 8}, EINVAL), ({"struct_size": 8}, EINVAL),
             ({"flip": 2}, EINVAL), ({"flip": -1}, EINVAL), ({"C": 1}, ERANGE), ({"C": 9}, ERANGE), ({"S": 0}, ERANGE), ({"S": 9}, ERANGE),
             ({"B": 64, "C": 8, "H": 1024, "W": 1024}, ERANGE),                                        # the summed map at 2 GiB
             ({"B": 256, "C": 2, "H": 1024, "W": 1024}, ERANGE),                                       # the mask at 2 GiB
             ({"h1": 16384, "w1": 16384}, ERANGE)]                                                     # a logits tensor beyond 2 GiB
    for kw, want in cases:
        assert raw_fold(zs, (B, H, W), True, probs, mask, conf, over=kw) == want, kw
    x = torch.randn(B, 3, H, W, device=DEV)
    out = torch.full((2 * B, 3, 8, 12), SENTINEL, device=DEV)
    assert L.uaps_tta_views(None) == EINVAL
    vfull = C.sizeof(_lib.TTAViewsCall)
    vcases = [({"x": None}, EINVAL), ({"out": None}, EINVAL), ({"B": 0}, EINVAL), ({"Cin": 0}, EINVAL), ({"H": 0}, EINVAL), ({"W": -1}, EINVAL),
              ({"h": 0}, EINVAL), ({"w": 0}, EINVAL), ({"flip": 2}, EINVAL), ({"struct_size": vfull - 8}, EINVAL), ({"struct_size": 4}, EINVAL),
              ({"B": 64, "Cin": 8, "H": 1024, "W": 1024}, ERANGE), ({"h": 16384, "w": 16384}, ERANGE)]
    for kw, want in vcases:
        assert raw_views(x, out, 8, 12, 1, over=kw) == want, kw
    torch.cuda.synchronize()
    assert bool((probs == SENTINEL).all()) and bool((mask == -7).all()) and bool((conf == SENTINEL).all())
    assert bool((out == SENTINEL).all())


def test_a_later_headers_struct_is_accepted():
    """A larger struct_size: this version's fields are read, what follows is not; the Python surface's bits come back."""
    from uaps_amd import _lib, tta_fold, tta_views
    case, zs_cpu, _ = R.reference("vec-32x48", True)
    zs = [z.to(DEV) for z in zs_cpu]
    want = tta_fold(zs, (case.H, case.W))

    class Later(C.Structure):
        _fields_ = [("base", _lib.TTAFoldCall), ("appended", C.c_double * 4)]
    probs, mask, conf = torch.empty_like(want.probs), torch.empty_like(want.mask), torch.empty_like(want.conf)
    assert raw_fold(zs, (case.B, case.H, case.W), True, probs, mask, conf, struct=Later()) == 0
    assert torch.equal(probs, want.probs) and torch.equal(mask, want.mask) and torch.equal(conf, want.conf)
    x = torch.randn(2, 3, 32, 48, device=DEV)
    out = torch.empty(4, 3, 24, 36, device=DEV)
    assert raw_views(x, out, 24, 36, 1, over={"struct_size": C.sizeof(_lib.TTAViewsCall) + 32}) == 0
    assert torch.equal(out, tta_views(x, (24, 36)))


@pytest.fixture(scope="module")
def net():
    import uaps_amd
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet_uaps", 3, 4)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)).to(DEV)
    return model.eval(), x


def _composed(model, x, sizes):
    """The reference's loop around forward_main, in float64 behind the network."""
    acc = None
    for size in sizes:
        cur = R.resize(x, size)
        for flipped in (False, True):
            z = model.forward_main(cur.flip(3) if flipped else cur).double()
            p = F.softmax(z, dim=1)
            p = R.resize(p.flip(3) if flipped else p, x.shape[-2:])
            acc = p if acc is None else acc + p
    return acc.cpu()


def test_wiring_on_the_real_network(net):
    from uaps_amd import inference, predict_tta, scaled_sizes, tta_fold, tta_views
    model, x = net
    sizes = scaled_sizes(64, 64, size_multiple=16)
    assert sizes == [(s, s) for s in (32, 48, 64, 96, 128)]
    with torch.no_grad():
        res = predict_tta(model, x)
        want = tta_fold([model.forward_main(tta_views(x, sz)) for sz in sizes], (64, 64))
        assert torch.equal(res.probs, want.probs) and torch.equal(res.mask, want.mask) and torch.equal(res.conf, want.conf)
        assert res.probs.shape == (2, 4, 64, 64) and res.mask.shape == (2, 64, 64)
        R.check_mask(res.mask, _composed(model, x, sizes))
        assert float((res.probs.sum(1) - 10).abs().max()) <= R.TAU_SUM
        one = predict_tta(model, x, scales=(1.0,), flip=False)
        p64 = F.softmax(model.forward_main(x).double(), dim=1).cpu()
        R.check_mask(one.mask, p64)
        clear = R.clear_pixels(p64)
        assert torch.equal(one.mask.cpu()[clear], inference.predict_main(model, x).cpu()[clear])


def test_evaluate_with_tta(net):
    from uaps_amd import inference
    model, x = net
    y = torch.randint(0, 4, (2, 64, 64), generator=torch.Generator().manual_seed(4)).to(DEV)
    batches = [(x, y), (x.flip(2), y)]
    plain, with_tta = inference.evaluate(model, batches), inference.evaluate(model, batches, tta=True)
    assert with_tta["images"] == plain["images"] == 4
    assert all(0.0 <= with_tta[k] <= 100.0 for k in ("mIoU(%)", "mDice(%)", "Accuracy(%)"))
    assert inference.evaluate(model, batches, tta=(1.0, 1.5))["images"] == 4


def test_res_uaps_forward_tta():
    import uaps_amd
    torch.manual_seed(0)
    model = uaps_amd.net_factory("resnet50_uaps", 3, 4, n_aux=1)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)).to(DEV)
    out = model(x, tta=True)
    assert out.shape == (2, 4, 64, 64) and out.dtype == torch.float32
    assert float((out.sum(1) - 10).abs().max()) <= R.TAU_SUM
    heads = model(x)
    assert isinstance(heads, tuple) and len(heads) == 2 and heads[0].shape == (2, 4, 64, 64)
    with torch.no_grad():                                  # the main-head-only path the TTA runs on: the same tensor as the first head
        assert torch.equal(model.forward_main(x), model(x)[0])
