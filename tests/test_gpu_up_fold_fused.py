"""-m gpu: the input gradient of up4's first convolution (3x3, 16 -> 16 + 16 channels on 256-wide maps) with the bilinear fold of its
up-sampled half as one full-width-row pass (csrc/up_bwd_row.hip, include/uaps_hip.h: uaps_up_bwd_fused) against the two launches it
replaces on the same operands -- uaps_conv_bwd_data_cat (conv_hr16x2_kernel) followed by uaps_up_cat_bwd (up_cat_bwd_low_kernel<32> /
<8>) -- through the C ABI in the fp16-split mode.  Those two launches are held against float64 by tests/test_gpu_conv_forms.py and
tests/test_gpu_resample_forms.py; equality carries their accuracy over.  Then: on the image border, the run boundary and the seam
between waves, outside its form, with a non-finite gradient, and inside a trainer step."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENOFORM, EINVAL = -4, -1
SENTINEL = -12345.678
PAD = 256             # sentinel floats either side of an output


@pytest.fixture(autouse=True)
def _h16_mode():
    """The kernel exists in the fp16-split arithmetic only: every test runs in that mode whatever an earlier test left behind."""
    from uaps_amd import conv
    conv.set_mode("h16")
    yield
    conv.set_mode("h16")


def _operands(B, H, kind, seed, W=256, C1=16, C2=16, Cout=16):
    """dy [B, Cout, H, W], the packed input-gradient weights of a [Cout, C1 + C2, 3, 3] convolution and the bound of |dy|."""
    from uaps_amd import bounds, conv
    g = torch.Generator().manual_seed(seed)
    if kind == "integer":                                  # every product and every sum of the convolution is exact
        dy = torch.randint(-8, 9, (B, Cout, H, W), generator=g).float()
        w = torch.randint(-3, 4, (Cout, C1 + C2, 3, 3), generator=g).float()
    else:
        dy = torch.randn(B, Cout, H, W, generator=g)
        w = torch.randn(Cout, C1 + C2, 3, 3, generator=g) / 10
    if kind.startswith("row"):                             # non-zero in one row only
        m = torch.zeros(H, W)
        m[int(kind[3:])] = 1
        dy = dy * m
    if kind == "seam":                                     # non-zero in columns 127 and 128 only: the seam between two waves' tiles
        m = torch.zeros(H, W)
        m[:, 127:129] = 1
        dy = dy * m
    dy, w = dy.to(DEV), w.to(DEV)
    dyb = (bounds.from_value(dy.abs().max() * 1.001 + 1e-30), 1.0)
    return dict(B=B, H=H, W=W, C1=C1, C2=C2, Cout=Cout, dy=dy, w=w, wb=conv.pack_weights(w)[1], dyb=dyb)


def _framed(shape):
    """An output as a view into a sentinel-filled buffer (16-byte aligned): (buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL, device=DEV)
    return buf, buf[PAD:PAD + n].view(shape)


def _frame_ok(buf, view):
    n = view.numel()
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + n:] == SENTINEL).all())


def _two_launches(s):
    from uaps_amd import _lib
    dev = torch.device(DEV)
    B, H, W, C1, C2, Cout = (s[k] for k in ("B", "H", "W", "C1", "C2", "Cout"))
    dx1 = torch.empty(B, C1, H, W, device=dev)
    dx2 = torch.empty(B, C2, H, W, device=dev)
    dlow = torch.empty(B, C2, H // 2, W // 2, device=dev)
    L = _lib.lib()
    with _lib.device_guard(dev):
        st = _lib.current_stream(dev)
        rc = L.uaps_conv_bwd_data_cat_h(_lib.mk_hints((s["dyb"],)), s["dy"].data_ptr(), s["wb"].data_ptr(), dx1.data_ptr(), C1, dx2.data_ptr(), C2,
                                        B, Cout, H, W, 3, 0, st)
        _lib.check(rc, "uaps_conv_bwd_data_cat")
        _lib.check(L.uaps_up_cat_bwd(dx2.data_ptr(), None, dlow.data_ptr(), B, 0, C2, H // 2, W // 2, st), "uaps_up_cat_bwd")
    return dx1, dlow


def _fused_raw(s, dskip, dlow, bound=True, dy=None, dskip_ptr=None):
    from uaps_amd import _lib
    dev = torch.device(DEV)
    with _lib.device_guard(dev):
        rc = _lib.lib().uaps_up_bwd_fused((dy if dy is not None else s["dy"]).data_ptr(), s["wb"].data_ptr(),
                                          s["dyb"][0].data_ptr() if bound else None, float(s["dyb"][1]),
                                          dskip_ptr if dskip_ptr is not None else dskip.data_ptr(), s["C1"], dlow.data_ptr(), s["C2"],
                                          s["B"], s["Cout"], s["H"], s["W"], 3, 0, _lib.current_stream(dev))
    torch.cuda.synchronize()
    return rc


def _check_equal(s):
    """The fused launch into framed, sentinel-filled outputs equals the two launches; nothing outside the outputs is written, nothing
    inside is left; a second launch into re-dirtied buffers gives the same bits."""
    ref_skip, ref_low = _two_launches(s)
    B, H, W, C1, C2 = (s[k] for k in ("B", "H", "W", "C1", "C2"))
    bs, dskip = _framed((B, C1, H, W))
    bl, dlow = _framed((B, C2, H // 2, W // 2))
    assert _fused_raw(s, dskip, dlow) == 0
    for name, a, b in (("d(skip)", dskip, ref_skip), ("d(low)", dlow, ref_low)):   # (the figures first: pytest shows them beside a failure)
        print(name, "differing", int((a != b).sum()), "of", a.numel(), "max |diff|", float((a.double() - b.double()).abs().max()))
    assert _frame_ok(bs, dskip) and _frame_ok(bl, dlow)
    assert not bool((dskip == SENTINEL).any()) and not bool((dlow == SENTINEL).any())
    assert torch.equal(dskip, ref_skip)
    assert torch.equal(dlow, ref_low)
    first = (dskip.clone(), dlow.clone())
    bs.fill_(SENTINEL + 1.0)
    bl.fill_(SENTINEL + 1.0)
    assert _fused_raw(s, dskip, dlow) == 0
    assert torch.equal(dskip, first[0]) and torch.equal(dlow, first[1])
    return dskip, dlow


# (B, H): one run, both image edges, no halo; a halo below the first run and above the second; a middle run with a halo on both sides
SHAPES = [(1, 16), (3, 32), (2, 48)]


@pytest.mark.parametrize("kind", ["random", "integer"])
@pytest.mark.parametrize("B,H", SHAPES)
def test_one_pass_equals_the_two_launches_and_repeats(B, H, kind):
    _check_equal(_operands(B, H, kind, seed=17 + B + H))


@pytest.mark.parametrize("row", [15, 16, 17])
def test_a_single_row_either_side_of_the_run_boundary(row):
    """dy non-zero in one row of H = 48 next to the boundary between the first two runs: a dropped or doubled halo contribution shows
    as a wrong low row 7 or 8."""
    s = _operands(2, 48, f"row{row}", seed=5)
    _, dlow = _check_equal(s)
    assert bool((dlow[:, :, 6:10] != 0).any())             # the rows around the boundary carry the gradient


def test_the_seam_between_waves():
    _check_equal(_operands(2, 32, "seam", seed=8))


def test_more_runs_than_workgroups():
    """H = 16 with more images than the launch has workgroups (one per CU): a workgroup walks through several runs."""
    from uaps_amd import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = max(cus, 256) + 3
    assert _lib.lib().uaps_up_bwd_fused_grid(B, 16) < B
    _check_equal(_operands(B, 16, "random", seed=29))


@pytest.mark.parametrize("what", ["W128", "H24", "low32", "no_dy_bound", "exact", "split", "misaligned"])
def test_outside_its_form_nothing_is_written(what):
    from uaps_amd import conv
    B, H, W, C2 = dict(W128=(2, 16, 128, 16), H24=(2, 24, 256, 16), low32=(2, 16, 256, 32)).get(what, (2, 16, 256, 16))
    s = _operands(B, H, "random", seed=3, W=W, C2=C2)
    bs, dskip = _framed((B, 16, H, W))
    bl, dlow = _framed((B, C2, H // 2, W // 2))
    try:
        if what in ("exact", "split"):
            conv.set_mode(what)
        rc = _fused_raw(s, dskip, dlow, bound=what != "no_dy_bound", dskip_ptr=dskip.data_ptr() + 4 if what == "misaligned" else None)
        assert rc in (ENOFORM, EINVAL)
        assert bool((bs == SENTINEL).all()) and bool((bl == SENTINEL).all())
        if what not in ("no_dy_bound", "misaligned"):
            assert not conv.up_bwd_eligible(s["dy"], 16, C2, 3)
        if what == "no_dy_bound":
            assert conv.up_bwd_fused(s["dy"], None, s["wb"], 16, C2, 0) is None
    finally:
        conv.set_mode("h16")


def test_a_non_finite_gradient_raises_the_error_word():
    """An inf planted in dy: UAPS_ERR_CONV_NONFINITE as conv_hr16x2_kernel raises it.  (The outputs are not compared: the seven-tap fold
    turns 0 * inf into NaN where the four-tap fold does not.)"""
    from uaps_amd import _lib
    s = _operands(2, 32, "random", seed=13)
    s["dy"][1, 3, 16, 100] = float("inf")
    err = _lib.error_word(torch.device(DEV))
    err.zero_()
    _two_launches(s)
    torch.cuda.synchronize()
    ref = int(err.item())
    err.zero_()
    _, dskip = _framed((2, 16, 32, 256))
    _, dlow = _framed((2, 16, 16, 128))
    assert _fused_raw(s, dskip, dlow) == 0
    got = int(err.item())
    err.zero_()
    assert ref & 1 and got == ref, (ref, got)


def test_trainer_step_with_the_switch_on_and_off():
    """One training step at 2 + 2 images of 32 x 256 (the smallest size at which the net takes this form), 4 classes, K = 3, with
    UAPS_FUSED_UP_FOLD on and off: the same loss, gradients and state (buffers, Adam moments, parameters) bit for bit; the fused kernel
    once per decoder, and as many launches fewer of the input-gradient kernel it replaces."""
    import uaps_amd
    from uaps_amd import conv, lazybn
    torch.manual_seed(6)
    m_on = uaps_amd.UNet_UAPS(3, 4, feature_chns=[16, 16, 32, 32, 64])
    m_off = copy.deepcopy(m_on)
    rng = np.random.default_rng(4)
    xl = torch.tensor(rng.standard_normal((2, 3, 32, 256)).astype(np.float32)).to(DEV)
    xu = torch.tensor(rng.standard_normal((2, 3, 32, 256)).astype(np.float32)).to(DEV)
    yl = torch.tensor(uaps_amd.data.synthetic_masks(rng, 2, 4, 32, 256)).to(DEV)
    res, names, opt = {}, {}, {}
    prev = conv._FUSED_UP_FOLD
    try:
        for on, m in ((True, m_on), (False, m_off)):
            conv._FUSED_UP_FOLD = on
            tr = uaps_amd.UAPSTrainer(m.to(DEV), base_lr=1e-3, seed=11)
            uaps_amd.perturb.manual_seed(7, 0)
            np.random.seed(7)
            conv.KERNEL_EVENTS, conv.EVENT_FILTER = {}, None
            res[on] = float(tr.train_step(xl, yl, xu)["loss"])
            names[on], conv.KERNEL_EVENTS = {k: len(v) for k, v in conv.KERNEL_EVENTS.items()}, None
            opt[on] = tr.optimizer
            lazybn.assert_none_pending()
    finally:
        conv._FUSED_UP_FOLD, conv.KERNEL_EVENTS = prev, None
    assert res[True] == res[False]
    for (n, ba), bb in zip(m_on.named_buffers(), m_off.buffers()):
        assert torch.equal(ba, bb), n
    for (n, pa), pb in zip(m_on.named_parameters(), m_off.parameters()):
        assert (pa.grad is None) == (pb.grad is None), n
        if pa.grad is not None:
            assert torch.equal(pa.grad, pb.grad), n
    sa, sb = opt[True].state_dict()["state"], opt[False].state_dict()["state"]
    assert sa.keys() == sb.keys() and len(sa) > 0
    for k in sa:
        assert torch.equal(sa[k]["exp_avg"], sb[k]["exp_avg"]) and torch.equal(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"]), k
    for (n, pa), pb in zip(m_on.named_parameters(), m_off.parameters()):
        assert torch.equal(pa, pb), n
    n_fused = names[True].get(conv.UP_BWD_KERNEL)
    assert n_fused == 4 and conv.UP_BWD_KERNEL not in names[False], (names[True], names[False])
    old = "conv_hr16x2_kernel"
    assert names[False].get(old, 0) >= 4 and names[True].get(old, 0) == names[False][old] - 4, (names[True], names[False])
