"""Hysteresis thresholding and binary reconstruction without a GPU: the package's CPU restatement (uaps_amd/hysteresis.py, a
union-find) against scipy (tests/hysteresis_ref.py), every refusal of the two functions, the C ABI's argument checks (they return before
any launch) and the hysteresis= keyword of inference.predict_instances / inference.evaluate around a stub network of four classes
with two heads and one of a single sigmoid channel.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import components_ref as CR
import hysteresis_ref as R
from conftest import ROOT
from test_morph_host import Stub, _batches, _host_confusion

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
PLANES = ((2, 16, 16), (2, 17, 65), (2, 37, 53), (2, 130, 161), (2, 3, 1100), (2, 256, 256))
LINES = ((2, 1, 1), (2, 1, 70), (2, 64, 1))


def _run(s, low, high, **kw):
    from uaps_amd import hysteresis
    src = torch.from_numpy(np.array(s))
    out = hysteresis(src, low, high, **kw)
    assert out.dtype == torch.int64 and out.shape == (src.shape[0],) + src.shape[2:]
    return out.numpy()


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("from_logits", (False, True), ids=("scores", "logits"))
@pytest.mark.parametrize("Cn", (4, 1), ids=("C4", "C1"))
def test_cpu_path_equals_scipy(Cn, from_logits, connectivity):
    for shape in PLANES:
        s = R.case(shape, Cn, from_logits)                      # (asserts the margin)
        for min_area in (1, 5):
            for per_class in ((False, True) if Cn == 4 else (False,)):
                ref = R.expected(shape, Cn, from_logits, per_class, connectivity, min_area)       # (asserts "informative")
                lo, hi = R.PER_CLASS if per_class else (R.LOW, R.HIGH)
                got = _run(s, lo, hi, from_logits=from_logits, connectivity=connectivity, min_area=min_area)
                assert np.array_equal(got, ref), (shape, min_area, per_class)


@pytest.mark.parametrize("connectivity", (4, 8))
def test_cpu_path_equals_scipy_on_one_pixel_rows_and_columns_without_the_informative_claim(connectivity):
    for shape in LINES:
        for Cn in (4, 1):
            for from_logits in (False, True):
                s = R.case(shape, Cn, from_logits)
                ref = R.expected(shape, Cn, from_logits, False, connectivity, 1, check=False)
                assert np.array_equal(_run(s, R.LOW, R.HIGH, from_logits=from_logits, connectivity=connectivity), ref), (shape, Cn)


def test_the_rule_on_a_hand_made_map():
    from uaps_amd import hysteresis
    s = torch.full((1, 3, 3, 7), 0.05)
    s[0, 1, 1, 0:3] = 0.4                                       # a weak run of class 1 with one strong pixel: kept whole
    s[0, 1, 1, 1] = 0.9
    s[0, 1, 1, 4:6] = 0.4                                       # a weak run without one: dropped
    s[0, 2, 1, 3] = 0.9                                         # a seed of class 2 between them joins neither
    s[0, 0] = 0.95                                              # the background's score takes no part
    out = hysteresis(s, 0.3, 0.6)
    assert out[0, 1].tolist() == [1, 1, 1, 2, 0, 0, 0] and int((out != 0).sum()) == 4
    assert hysteresis(s, 0.3, 0.6, classes=(1,))[0, 1].tolist() == [1, 1, 1, 0, 0, 0, 0]
    assert hysteresis(s, 0.3, 0.6, min_area=2)[0, 1].tolist() == [1, 1, 1, 0, 0, 0, 0]
    assert hysteresis(s, (0.3, 0.3), (0.95, 0.6))[0, 1].tolist() == [0, 0, 0, 2, 0, 0, 0]
    assert hysteresis(s, (0.3, 0.95), (0.6, 0.95), classes=(2, 1))[0, 1].tolist() == [0, 0, 0, 2, 0, 0, 0]      # thresholds follow `classes`
    assert hysteresis(s, 0.3, 0.6, background=2, classes=(0, 1))[0, 1].tolist() == [0] * 7                       # class 0 wins everywhere
    t = s.clone()
    t[0, 2, 1, 1] = 0.9                                         # a tie of classes 1 and 2 on the seed: the lowest class
    assert hysteresis(t, 0.3, 0.6)[0, 1].tolist() == [1, 1, 1, 2, 0, 0, 0]
    t[0, 2, 1, 2] = float("nan")                                # a NaN among the selected scores: neither candidate nor seed
    assert hysteresis(t, 0.3, 0.6)[0, 1].tolist() == [1, 1, 0, 2, 0, 0, 0]
    assert hysteresis(t, 0.3, 0.6, classes=(1,))[0, 1].tolist() == [1, 1, 1, 0, 0, 0, 0]       # ... of the SELECTED scores
    assert (hysteresis(s, 0.3, float("inf")) == 0).all() and (hysteresis(s, float("-inf"), float("-inf")) != 0).all()
    one = s[:, 1:2]
    assert hysteresis(one, 0.3, 0.6)[0, 1].tolist() == [1, 1, 1, 0, 0, 0, 0]
    assert torch.equal(hysteresis(torch.log(one / (1 - one)), 0.3, 0.6, from_logits=True), hysteresis(one, 0.3, 0.6))


def test_reconstruct_equals_scipy_and_its_properties():
    from uaps_amd import components, hysteresis, reconstruct
    for shape in PLANES[:4]:
        m = np.array(CR.rings(*shape))
        rng = np.random.default_rng(5)
        mk = rng.random(m.shape) < 0.03
        mt, kt = torch.from_numpy(m), torch.from_numpy(mk)
        for connectivity in (4, 8):
            for kw in ({}, {"classes": (3, 1)}, {"background": 2}, {"min_area": 5}):
                ref = R.reconstruct(m, mk, 4, connectivity=connectivity, **kw)
                got = reconstruct(mt, kt, 4, connectivity=connectivity, **kw)
                assert got is not mt and np.array_equal(got.numpy(), ref), (shape, kw)
                assert np.array_equal(got.numpy() == 255, m == 255)                         # ignore labels pass through
                assert torch.equal(reconstruct(got, kt, 4, connectivity=connectivity, **kw), got)      # idempotent
            assert (ref != m).any() and (ref != 0).any()
            assert torch.equal(reconstruct(mt, kt.to(torch.uint8) * 7, 4, connectivity=connectivity), reconstruct(mt, kt, 4, connectivity=connectivity))
            assert torch.equal(reconstruct(mt, torch.ones_like(kt), 4, connectivity=connectivity), mt)
            none = reconstruct(mt, torch.zeros_like(kt), 4, connectivity=connectivity, classes=(1, 3))
            assert torch.equal(none, torch.where((mt == 1) | (mt == 3), torch.zeros_like(mt), mt))
            # hysteresis is reconstruction of the candidate mask from the seed mask
            s = R.case(shape, 4, False)
            cls, cand, seed = R.classify(s, R.LOW, R.HIGH)
            cmask = torch.from_numpy(np.where(cand, cls, 0))
            hyst = hysteresis(torch.from_numpy(np.array(s)), R.LOW, R.HIGH, connectivity=connectivity)
            assert torch.equal(hyst, reconstruct(cmask, torch.from_numpy(seed), 4, connectivity=connectivity))
            assert torch.equal(hysteresis(torch.from_numpy(np.array(s)), R.LOW, R.HIGH, connectivity=connectivity, min_area=5),
                               components(hyst, [("area_open", 5)], 4, connectivity=connectivity))


def test_argument_checks():
    from uaps_amd import hysteresis, reconstruct
    s = torch.full((1, 4, 4, 4), 0.25)
    assert hysteresis(s, 0.2, 0.5).shape == (1, 4, 4)
    for bad in (s.double(), s[0], s.long(), s.numpy()):
        with pytest.raises(TypeError):
            hysteresis(bad, 0.2, 0.5)
    for low, high in ((0.6, 0.5), (float("nan"), 0.5), (0.2, float("nan")), ((0.2, 0.2), 0.5), (0.2, (0.5,) * 4), ("a", 0.5), (None, 0.5),
                      ((0.2, 0.7, 0.2), (0.5, 0.6, 0.5))):
        with pytest.raises(ValueError, match="hysteresis: "):
            hysteresis(s, low, high)
    for kw in ({"classes": ()}, {"classes": (1, 1)}, {"classes": (0,)}, {"classes": (4,)}, {"classes": (-1,)}, {"connectivity": 5},
               {"background": 2 ** 31}, {"min_area": 0}, {"min_area": 1.5}, {"min_area": True}):
        with pytest.raises(ValueError, match="hysteresis: "):
            hysteresis(s, 0.2, 0.5, **kw)
    with pytest.raises(ValueError):
        hysteresis(torch.zeros(1, 9, 4, 4), 0.2, 0.5)
    with pytest.raises(ValueError):
        hysteresis(torch.zeros(0, 4, 4, 4), 0.2, 0.5)
    one = torch.zeros(1, 1, 4, 4)
    assert hysteresis(one, 0.2, 0.5, classes=[1]).shape == (1, 4, 4)
    for kw in ({"classes": (0,)}, {"background": 1}, {"classes": (2,)}):
        with pytest.raises(ValueError, match="hysteresis: "):
            hysteresis(one, 0.2, 0.5, **kw)
    assert hysteresis(s, float("-inf"), float("inf")).eq(0).all()
    m, k = torch.zeros(1, 4, 4, dtype=torch.int64), torch.zeros(1, 4, 4, dtype=torch.bool)
    assert reconstruct(m, k, 4) is not m
    for bad_m, bad_k in ((m.int(), k), (m[0], k[0]), (m, k.long()), (m, k.float()), (m.numpy(), k), (m, k.numpy())):
        with pytest.raises(TypeError):
            reconstruct(bad_m, bad_k, 4)
    with pytest.raises(ValueError, match="reconstruct: "):
        reconstruct(m, k[:, :2], 4)
    for kw in ({"classes": ()}, {"classes": (1, 1)}, {"classes": (0,)}, {"classes": (4,)}, {"connectivity": 5}, {"background": -2 ** 31 - 1},
               {"min_area": 0}):
        with pytest.raises(ValueError, match="reconstruct: "):
            reconstruct(m, k, 4, **kw)
    with pytest.raises(ValueError):
        reconstruct(m, k, 9)
    with pytest.raises(ValueError):
        reconstruct(m[:0], k[:0], 4)


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib
    new = {"uaps_hysteresis", "uaps_hysteresis_workspace_bytes"}
    text = open(os.path.join(ROOT, "include", "uaps_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    assert new <= declared and new <= set(_lib.SIGNATURES)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in new:
        assert hasattr(raw, n), n
    assert _lib.lib().uaps_abi_version() == 3
    body = re.search(r"typedef struct uaps_hysteresis_call \{(.*?)\} uaps_hysteresis_call;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.HysteresisCall._fields_], names
    defines = dict(re.findall(r"#define (UAPS_HYST_[A-Z_]+) (\d+)", text))
    assert int(defines["UAPS_HYST_MAX_CLASSES"]) == _lib.HYST_MAX_CLASSES == 8
    assert C.sizeof(_lib.HysteresisCall) == 8 + 4 * 4 + 2 * 4 + 3 * 32 + 3 * 4 + 4 + 7 * 8      # (4 bytes of padding before the pointers)


def _call(marker=False, **kw):
    from uaps_amd import _lib
    c = _lib.HysteresisCall()
    c.struct_size = C.sizeof(_lib.HysteresisCall)
    c.B, c.C, c.H, c.W, c.n_classes, c.background, c.connectivity, c.min_area = 1, 4, 8, 8, 2, 0, 8, 1
    c.classes[0], c.classes[1] = 1, 2
    c.low[0], c.low[1], c.high[0], c.high[1] = 0.25, 0.25, 0.5, 0.5
    c.out, c.workspace, c.workspace_bytes = 8192, 65536, 1 << 20        # never dereferenced: every call returns before a launch
    if marker:
        c.mask, c.markers = 4096, 16384
    else:
        c.scores = 4096
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    return c


def test_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()
    run = lambda c: L.uaps_hysteresis(C.byref(c))
    nan, inf = float("nan"), float("inf")
    assert L.uaps_hysteresis(None) == EINVAL
    assert run(_call(scores=None)) == EINVAL                                                 # neither form's operands
    assert run(_call(out=None)) == EINVAL and run(_call(workspace=None)) == EINVAL
    assert run(_call(mask=16384)) == EINVAL and run(_call(markers=16384)) == EINVAL         # both forms' operands
    assert run(_call(True, mask=None)) == EINVAL and run(_call(True, markers=None)) == EINVAL
    assert run(_call(True, out=4096)) == EINVAL                                              # out == mask
    for marker in (False, True):
        for dim in ("B", "H", "W"):
            assert run(_call(marker, **{dim: 0})) == EINVAL and run(_call(marker, **{dim: -3})) == EINVAL
        assert run(_call(marker, connectivity=5)) == EINVAL and run(_call(marker, connectivity=0)) == EINVAL
        assert run(_call(marker, min_area=0)) == EINVAL
        assert run(_call(marker, n_classes=0)) == EINVAL and run(_call(marker, n_classes=9)) == EINVAL
        assert run(_call(marker, classes=[1, 1])) == EINVAL and run(_call(marker, classes=[2, 1])) == EINVAL    # not strictly ascending
        assert run(_call(marker, classes=[0, 1])) == EINVAL and run(_call(marker, background=2)) == EINVAL      # the background
        assert run(_call(marker, classes=[-1, 1])) == EINVAL
        assert run(_call(marker, struct_size=C.sizeof(_lib.HysteresisCall) - 8)) == EINVAL    # a header without `stream`
        assert run(_call(marker, H=65536, W=32768)) == ERANGE                                 # H * W = 2^31
        assert run(_call(marker, B=64, H=2048, W=2048)) == ERANGE                             # B * H * W * 8 = 2 GiB
        assert run(_call(marker, B=8, H=4096, W=4096, workspace_bytes=1 << 40)) == ERANGE     # the workspace: 16 bytes a pixel
    assert run(_call(low=[0.6])) == EINVAL and run(_call(low=[0.25, 0.7])) == EINVAL         # low > high
    assert run(_call(low=[nan])) == EINVAL and run(_call(high=[0.5, nan])) == EINVAL         # a NaN threshold
    assert run(_call(from_logits=2)) == EINVAL
    assert run(_call(classes=[1, 4])) == EINVAL                                              # a class outside [0, C)
    assert run(_call(C=1)) == EINVAL and run(_call(C=1, n_classes=1, classes=[0], background=1)) == EINVAL       # C == 1: class 1 alone
    assert run(_call(C=0)) == ERANGE and run(_call(C=9)) == ERANGE
    assert run(_call(B=4, C=8, H=4096, W=4096, workspace_bytes=1 << 40)) == ERANGE           # scores of 2 GiB
    need = C.c_size_t()
    assert L.uaps_hysteresis_workspace_bytes(1, 8, 8, C.byref(need)) == 0 and need.value == 512 + 2 * 256 and need.value % 256 == 0
    for marker in (False, True):
        assert run(_call(marker, workspace_bytes=need.value - 1)) == EWORKSPACE               # too small
        assert run(_call(marker, workspace=65536 + 128)) == EWORKSPACE                        # misaligned
    assert L.uaps_hysteresis_workspace_bytes(1, 8, 8, None) == EINVAL and L.uaps_hysteresis_workspace_bytes(0, 8, 8, C.byref(need)) == EINVAL
    assert L.uaps_hysteresis_workspace_bytes(1, 65536, 32768, C.byref(need)) == ERANGE
    assert L.uaps_hysteresis_workspace_bytes(8, 4096, 4096, C.byref(need)) == ERANGE
    big = C.c_size_t()
    assert L.uaps_hysteresis_workspace_bytes(2, 1024, 1024, C.byref(big)) == 0 and big.value == 2 ** 21 * 16
    # +-inf thresholds, low == high and C == 1 with its one class pass every check: what refuses them is the workspace alone
    ok = dict(workspace_bytes=need.value - 1)
    assert run(_call(low=[-inf, 0.5], high=[inf, 0.5], **ok)) == EWORKSPACE
    assert run(_call(C=1, n_classes=1, classes=[1], **ok)) == EWORKSPACE
    assert run(_call(True, low=[nan, 0.7], C=0, from_logits=7, **ok)) == EWORKSPACE          # the marker form reads none of these


HYST = (0.3, 0.6)
BIN = (0.15, 0.3)                       # for the one-channel stub, whose sigmoid stays below 0.56


def _host_uncertainty(main, aux):
    """A host stand-in for consistency.uncertainty_map (a device kernel): both sides of a comparison go through it."""
    la, lm = torch.log_softmax(aux, dim=1), torch.log_softmax(main, dim=1)
    return (la.exp() * (la - lm)).sum(dim=1)


def test_predict_instances_with_hysteresis(monkeypatch):
    from uaps_amd import components, consistency, hysteresis, inference, label_instances, morphology
    monkeypatch.setattr(consistency, "uncertainty_map", _host_uncertainty)
    net = Stub(3, 4, heads=2)
    x = _batches(Stub(3, 4), 1)[0][0]
    main, aux = net(x)
    argmax = inference.predict(net, x)[0]
    hmask = hysteresis(main, *HYST, from_logits=True)
    assert not torch.equal(hmask, argmax) and (hmask != 0).any()
    assert not torch.equal(hmask, hysteresis(main, HYST[0], HYST[0], from_logits=True))      # something was dropped
    assert not torch.equal(hmask, hysteresis(main, HYST[1], HYST[1], from_logits=True))      # something grew beyond its seeds
    assert ((hmask != 0) & (argmax == 0)).any()                  # a candidate whose overall arg-max is the background
    maps = (torch.softmax(main, dim=1).amax(dim=1), consistency.uncertainty_map(main, aux))
    plain = inference.predict_instances(net, x)
    assert all(torch.equal(a, b) for a, b in zip(inference.predict_instances(net, x, hysteresis=None)[:3], plain[:3]))
    res, ref = inference.predict_instances(net, x, hysteresis=HYST), label_instances(hmask, maps)
    for a, b in zip(res[:3], ref[:3]):
        assert torch.equal(a, b)
    assert not torch.equal(res.labels, plain.labels)
    # the call's connectivity and a dict of keywords; the clean-up chains come after
    kw = {"low": (0.3, 0.25, 0.3), "high": (0.6, 0.5, 0.6), "min_area": 3}
    h4 = hysteresis(main, from_logits=True, connectivity=4, **kw)
    assert not torch.equal(h4, hmask)
    res, ref = inference.predict_instances(net, x, hysteresis=kw, connectivity=4), label_instances(h4, maps, connectivity=4)
    for a, b in zip(res[:3], ref[:3]):
        assert torch.equal(a, b)
    morph, steps = [("close", "square", 1)], [("area_open", 4)]
    both = components(morphology(hmask, morph, 4), steps, 4)
    assert not torch.equal(both, hmask)
    res, ref = inference.predict_instances(net, x, hysteresis=HYST, cleanup=morph, components=steps), label_instances(both, maps)
    for a, b in zip(res[:3], ref[:3]):
        assert torch.equal(a, b)
    shaped = inference.predict_instances(net, x, hysteresis=HYST, shapes=True, contours=True)
    assert torch.equal(shaped.also.instances.labels, label_instances(hmask, maps).labels)
    # under tta and tiled the mask comes from the probability maps
    from uaps_amd.tiled import predict_tiled
    from uaps_amd.tta import predict_tta
    t = predict_tta(net, x, scales=(1.0, 0.5), want=("probs", "conf"))
    tm = hysteresis(t.probs, 0.3 * 4, 0.6 * 4, connectivity=4)                              # (the sum over four views)
    res = inference.predict_instances(net, x, tta=(1.0, 0.5), hysteresis=(0.3 * 4, 0.6 * 4), connectivity=4)
    assert torch.equal(res.labels, label_instances(tm, (t.conf,), connectivity=4).labels) and (tm != 0).any()
    tl = predict_tiled(net, x, tile=16, overlap=4, want=("probs", "conf"))
    tm = hysteresis(tl.probs, *HYST)
    res = inference.predict_instances(net, x, tiled={"tile": 16, "overlap": 4, "uncertainty": None}, hysteresis=HYST)
    assert torch.equal(res.labels, label_instances(tm, (tl.conf,)).labels) and (tm != 0).any()
    for bad in (0.5, (0.3,), (0.3, 0.6, 0.9), "ab", {"low": 0.3}, {"low": 0.3, "high": 0.6, "connectivity": 4}, {"low": 0.3, "high": 0.6, "from_logits": True},
                (0.6, 0.3), (float("nan"), 0.6)):
        with pytest.raises(ValueError):
            inference.predict_instances(net, x, hysteresis=bad)


def test_one_channel_models(monkeypatch):
    from uaps_amd import consistency, hysteresis, inference, label_instances, skeletonize

    def never(*a):
        raise AssertionError("no uncertainty map is formed for a one-channel model")
    monkeypatch.setattr(consistency, "uncertainty_map", never)
    net = Stub(3, 1, heads=2)
    x = _batches(Stub(3, 4), 1)[0][0]
    main, _ = net(x)
    p = torch.sigmoid(main)[:, 0]
    hmask = hysteresis(main, *BIN, from_logits=True)
    assert set(hmask.unique().tolist()) == {0, 1}
    assert not torch.equal(hmask, (p >= BIN[0]).long()) and not torch.equal(hmask, (p >= BIN[1]).long())
    res = inference.predict_instances(net, x, hysteresis=BIN)
    ref = label_instances(hmask, (torch.maximum(p, 1 - p),))                               # no uncertainty map, though there is an auxiliary head
    for a, b in zip(res[:3], ref[:3]):
        assert torch.equal(a, b)
    assert int(res.count.sum()) > 0 and res.table.shape == ref.table.shape
    # later steps see two classes
    steps = [("area_open", 3), ("fill_holes", None)]
    from uaps_amd import components
    clean = components(hmask, steps, 2)
    assert not torch.equal(clean, hmask)
    res = inference.predict_instances(net, x, hysteresis=BIN, components=steps, skeleton=True, shapes=True)
    assert torch.equal(res.instances.labels, label_instances(clean, (torch.maximum(p, 1 - p),)).labels)
    assert torch.equal(res.skeleton.mask, skeletonize(clean, 2).mask) and res.skeleton.classes == (1,)
    with pytest.raises(ValueError, match="hysteresis="):
        inference.predict_instances(net, x)
    with pytest.raises(ValueError):
        inference.predict_instances(net, x, hysteresis=BIN, tta=True)
    with pytest.raises(ValueError):
        inference.predict_instances(net, x, hysteresis=BIN, tiled={"tile": 16, "overlap": 4})
    with pytest.raises(ValueError):
        inference.predict_instances(net, x, hysteresis={"low": 0.15, "high": 0.3, "classes": (0,)})
    with pytest.raises(ValueError, match="evaluate: "):
        inference.evaluate(net, [(x, torch.zeros(x.shape[0], *x.shape[2:], dtype=torch.int64))], hysteresis=BIN)


def test_evaluate_with_hysteresis(monkeypatch):
    from uaps_amd import components, hysteresis, inference, metrics
    monkeypatch.setattr(metrics, "seg_confusion_per_image", _host_confusion)
    net = Stub(3, 4, heads=2)
    batches = _batches(Stub(3, 4))
    plain = inference.evaluate(net, batches)
    assert list(plain) == ["mIoU(%)", "mDice(%)", "Accuracy(%)", "images"]                  # the dict of before
    assert inference.evaluate(net, batches, hysteresis=None) == plain
    steps = [("area_open", 4)]
    out = inference.evaluate(net, batches, hysteresis=HYST)
    kw = {"low": 0.3, "high": 0.6, "connectivity": 4, "min_area": 2}
    out4 = inference.evaluate(net, batches, hysteresis=kw)
    both = inference.evaluate(net, batches, hysteresis=HYST, components=steps)
    for d in (out, out4, both):
        assert set(d) - set(plain) == {"mIoU_clean(%)", "mDice_clean(%)"} and all(d[k] == plain[k] for k in plain)

    def clean_scores(chain):
        miou, mdice = [], []
        with torch.no_grad():
            for x, y in batches:
                clean = chain(net(x)[0])
                for b in range(len(y)):
                    cm = torch.bincount(y[b].flatten() * 4 + clean[b].flatten(), minlength=16).view(4, 4)
                    m = metrics.metrics_from_confusion(cm)
                    miou.append(m["miou"]); mdice.append(m["mdice"])
        return float(np.mean(miou) * 100), float(np.mean(mdice) * 100)

    assert (out["mIoU_clean(%)"], out["mDice_clean(%)"]) == clean_scores(lambda z: hysteresis(z, *HYST, from_logits=True))
    assert (out4["mIoU_clean(%)"], out4["mDice_clean(%)"]) == clean_scores(lambda z: hysteresis(z, from_logits=True, **kw))
    assert (both["mIoU_clean(%)"], both["mDice_clean(%)"]) == clean_scores(lambda z: components(hysteresis(z, *HYST, from_logits=True), steps, 4))
    assert len({out["mIoU_clean(%)"], out4["mIoU_clean(%)"], both["mIoU_clean(%)"], plain["mIoU(%)"]}) == 4
    inst = inference.evaluate(net, batches, instances={"max_instances": 4096})
    with_inst = inference.evaluate(net, batches, instances={"max_instances": 4096}, hysteresis=HYST)
    assert with_inst["defects_gt"] == inst["defects_gt"] and with_inst["defects_pred"] != inst["defects_pred"]
    assert all(with_inst[k] == out[k] for k in out)
    for bad in (0.5, {"low": 0.3}, {"low": 0.3, "high": 0.6, "from_logits": True}, (0.6, 0.3)):
        with pytest.raises(ValueError):
            inference.evaluate(net, batches, hysteresis=bad)
