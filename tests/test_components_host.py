"""Component clean-up without a GPU: the package's CPU restatement (uaps_amd/components.py, a union-find) against scipy
(tests/components_ref.py), the combine rule of hole filling, the C ABI's argument checks (they return before any launch) and the
components= keyword of inference.predict_instances / inference.evaluate around a stub network.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import components_ref as R
from conftest import ROOT
from test_morph_host import Stub, _batches, _host_confusion

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
PLANES = ((37, 53), (16, 16), (17, 65))                 # every case is asserted to be informative on each of them
LINES = ((1, 70), (64, 1))                              # no holes, every pixel on the border
STEPS = ([("area_open", n) for n in (1, 2, 5, 50)] + [("clear_border",)] + [("fill_holes", n) for n in (1, 2, 5, 50, None)])
_ids = lambda s: "-".join(str(v) for v in s)


def _run(m, steps, num_classes=4, **kw):
    from uaps_amd import components
    src = torch.from_numpy(np.array(m))
    out = components(src, steps, num_classes, **kw)
    assert out.dtype == torch.int64 and out.shape == src.shape and out is not src
    return out.numpy()


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("step", STEPS, ids=_ids)
def test_cpu_path_equals_scipy(step, connectivity):
    for H, W in PLANES:
        m = R.rings(2, H, W)
        ref = R.components(m, [step], 4, connectivity=connectivity)
        if step == ("area_open", 1):
            assert np.array_equal(ref, m)               # the identity, by definition: nothing to be informative about
        else:
            assert R.informative(ref, m), ("a vacuous case", H, W)
        assert np.array_equal(_run(m, [step], connectivity=connectivity), ref), (H, W)


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("step", STEPS, ids=_ids)
def test_cpu_path_equals_scipy_on_single_rows_and_columns_without_the_informative_claim(step, connectivity):
    for H, W in LINES:
        m = R.rings(2, H, W)
        ref = R.components(m, [step], 4, connectivity=connectivity)
        if step[0] == "fill_holes":
            assert np.array_equal(ref, m)               # a line has no holes
        if step[0] == "clear_border":
            assert (ref[m < 4] == 0).all()              # and every pixel on the border
        assert np.array_equal(_run(m, [step], connectivity=connectivity), ref), (H, W)


CHAINS = ([("area_open", 5), ("fill_holes", 50)],
          [("fill_holes", None), ("clear_border",), ("area_open", 50)],
          [("clear_border",), ("fill_holes", 5), ("area_open", 2), ("fill_holes", None)])


@pytest.mark.parametrize("steps", CHAINS, ids=("2", "3", "4"))
def test_chains_equal_their_steps_one_at_a_time(steps):
    for connectivity in (4, 8):
        m = R.rings(2, 37, 53)
        ref = R.components(m, steps, 4, connectivity=connectivity)
        assert R.informative(ref, m)
        one, seen = np.array(m), []
        for s in steps:
            nxt = _run(one, [s], connectivity=connectivity)
            seen.append(not np.array_equal(nxt, one))
            one = nxt
        assert all(seen), seen                          # every step of the chain had something to do
        assert np.array_equal(_run(m, steps, connectivity=connectivity), ref) and np.array_equal(one, ref)


def test_class_subsets_and_a_non_zero_background():
    m = np.array(R.rings(2, 37, 53))
    m[:, 30:33, 40:43] = 7                              # a value >= num_classes
    for steps in ([("area_open", 5)], [("clear_border",)], [("fill_holes", None)], [("fill_holes", 5), ("area_open", 50)]):
        for kw in ({}, {"classes": (2,)}, {"classes": (3, 1)}, {"background": 2}, {"background": 3, "classes": (0, 1)}):
            ref = R.components(m, steps, 4, **kw)
            got = _run(m, steps, **kw)
            assert np.array_equal(got, ref), (steps, kw)
            assert (ref != m).any(), (steps, kw)
            assert np.array_equal(got == 255, m == 255) and np.array_equal(got == 7, m == 7)
            bg = kw.get("background", 0)
            for c in range(4):
                if c != bg and c not in kw.get("classes", [k for k in range(4) if k != bg]):
                    assert np.array_equal(got == c, m == c), (steps, kw, c)         # an unselected class is neither lost nor grown


def test_checkerboard():
    m = R.checkerboard(9, 12)
    got = _run(m, [("fill_holes", None)], connectivity=8)       # the complement is 4-connected: every interior background pixel
    want = np.array(m)                                          # is a one-pixel hole
    want[0, 1:-1, 1:-1] = 1
    assert np.array_equal(got, want) and np.array_equal(got, R.components(m, [("fill_holes", None)], 4, connectivity=8))
    assert np.array_equal(got, _run(m, [("fill_holes", 1)], connectivity=8))
    edge = np.ones((9, 12), dtype=bool)
    edge[1:-1, 1:-1] = False
    assert np.array_equal(got[0][edge], m[0][edge]) and (m[0][edge] == 0).any()      # none on the border
    # under connectivity 4 the complement is ONE 8-connected component that touches the border
    assert np.array_equal(_run(m, [("fill_holes", None)], connectivity=4), m)
    assert np.array_equal(R.components(m, [("fill_holes", None)], 4, connectivity=4), m)


def test_nested_rings():
    m = R.nested_rings()
    for connectivity in (4, 8):
        got = _run(m, [("fill_holes", None)], connectivity=connectivity)
        assert np.array_equal(got, R.components(m, [("fill_holes", None)], 4, connectivity=connectivity))
        assert (got[0, 7:-7, 7:-7] == 1).all() and (m[0, 7:-7, 7:-7] == 0).all()     # inside the inner ring: class 1 (the smaller)
        between = np.zeros(m.shape[1:], dtype=bool)
        between[4:-4, 4:-4] = True
        between[5:-5, 5:-5] = False
        assert (m[0][between] == 0).all() and (got[0][between] == 2).all()          # between the rings: only a hole of class 2
        assert np.array_equal(got == 1, (m == 1) | (got != m) & ~between[None])      # the inner ring's own pixels stay class 1
        assert (got[0][m[0] == 1] == 1).all() and (got[0][m[0] == 2] == 2).all()
        assert (got[0, :2] == 0).all() and (got[0, :, :2] == 0).all()               # outside: untouched
        only2 = _run(m, [("fill_holes", None)], classes=(2,), connectivity=connectivity)
        assert (only2[0, 7:-7, 7:-7] == 2).all() and (only2[0][m[0] == 1] == 1).all()


def test_obstacles_inside_a_hole_stay_and_count_towards_its_area():
    m = np.zeros((1, 12, 13), dtype=np.int64)
    m[0, 2:10, 2:11] = 1
    m[0, 4:8, 4:9] = 0                                  # a 4 x 5 hole: 20 pixels ...
    m[0, 5, 5] = 255                                    # ... of which an ignore pixel
    m[0, 6, 6:8] = 3                                    # ... and a blob of an unselected class: 17 background pixels
    kw = {"classes": (1,)}
    for n, filled in ((16, False), (17, False), (19, False), (20, True), (None, True)):       # 17 <= n < 20 separates the two readings
        got = _run(m, [("fill_holes", n)], **kw)
        assert np.array_equal(got, R.components(m, [("fill_holes", n)], 4, **kw)), n
        assert (got != m).any() == filled, n
        assert got[0, 5, 5] == 255 and (got[0, 6, 6:8] == 3).all()
        if filled:
            assert int((got == 1).sum()) == int((m == 1).sum()) + 17
    # with class 3 selected too its blob is still no background: it stays, and has no hole of its own
    got = _run(m, [("fill_holes", None)])
    assert (got[0, 6, 6:8] == 3).all() and int((got == 1).sum()) == int((m == 1).sum()) + 17


def test_a_hole_that_reaches_the_border_through_one_pixel_is_not_filled():
    m = np.zeros((1, 9, 9), dtype=np.int64)
    m[0, 0:7, 1:8] = 1
    m[0, 2:5, 3:6] = 0
    closed = _run(m, [("fill_holes", None)])
    assert (closed[0, 2:5, 3:6] == 1).all()
    m[0, 0:2, 4] = 0                                    # a one-pixel channel to row 0
    for connectivity in (4, 8):
        assert np.array_equal(_run(m, [("fill_holes", None)], connectivity=connectivity), m)
        assert np.array_equal(R.components(m, [("fill_holes", None)], 4, connectivity=connectivity), m)
    m[0, 0, 4] = 1                                      # sealed again, one pixel lower
    assert (_run(m, [("fill_holes", None)])[0, 1:5, 3:6] == 1).all()
    d = np.zeros((1, 7, 7), dtype=np.int64)             # a diagonal leak: open to an 8-connected complement only
    d[0, 1:6, 1:6] = 1
    d[0, 2:4, 2:4] = 0
    d[0, 1, 1] = 0
    assert np.array_equal(_run(d, [("fill_holes", None)], connectivity=4), d)            # the complement is 8-connected: leaks
    assert (_run(d, [("fill_holes", None)], connectivity=8)[0, 2:4, 2:4] == 1).all()     # 4-connected: a hole


@pytest.mark.parametrize("n", (2, 5, 50))
def test_area_open_agrees_with_label_instances_min_area(n):
    from uaps_amd import components, label_instances
    for connectivity in (4, 8):
        m = torch.from_numpy(np.array(R.rings(2, 37, 53)))
        m[m == 255] = 0
        opened = components(m, [("area_open", n)], 4, connectivity=connectivity)
        a = label_instances(opened, connectivity=connectivity, max_instances=512)
        b = label_instances(m, connectivity=connectivity, min_area=n, max_instances=512)
        assert int(b.count.max()) <= 512 and int(b.count.sum()) < int(label_instances(m, connectivity=connectivity).count.sum())
        assert torch.equal(a.labels, b.labels) and torch.equal(a.count, b.count) and torch.equal(a.table, b.table)
        assert torch.equal(opened, torch.where(b.labels > 0, m, torch.zeros_like(m)))


def test_area_open_one_is_the_identity():
    for H, W in PLANES + LINES + ((1, 1),):
        m = R.rings(2, H, W)
        for connectivity in (4, 8):
            assert np.array_equal(_run(m, [("area_open", 1)], connectivity=connectivity), m)


def test_argument_checks():
    from uaps_amd import components
    from uaps_amd.components import check_steps
    m = torch.zeros(1, 4, 4, dtype=torch.int64)
    ok = [("area_open", 2)]
    assert components(m, ok, 4) is not m
    assert check_steps([["fill_holes", None], ("clear_border",), ("area_open", np.int64(3))]) == \
        (("fill_holes", None), ("clear_border",), ("area_open", 3))
    for bad in (m.int(), m[0], m.float(), np.zeros((1, 4, 4), dtype=np.int64)):
        with pytest.raises(TypeError):
            components(bad, ok, 4)
    for steps in ([], ok * 9, "area_open", 3, [("melt", 1)], ["area_open"], [("area_open",)], [("area_open", 0)], [("area_open", -1)],
                  [("area_open", 1.5)], [("area_open", None)], [("area_open", True)], [("area_open", 2, 3)], [("clear_border", 1)],
                  [("fill_holes",)], [("fill_holes", 0)], [("fill_holes", "all")], [()], [("open", "disk", 1)]):
        with pytest.raises(ValueError, match="components: "):
            components(m, steps, 4)
    for kw in ({"classes": ()}, {"classes": (1, 1)}, {"classes": (0,)}, {"classes": (4,)}, {"classes": (-1,)},
               {"classes": tuple(range(1, 10))}, {"connectivity": 6}, {"background": 2 ** 31}):
        with pytest.raises(ValueError):
            components(m, ok, 4, **kw)
    with pytest.raises(ValueError):
        components(m, ok, 9)
    with pytest.raises(ValueError):
        components(torch.zeros(0, 4, 4, dtype=torch.int64), ok, 4)
    with pytest.raises(ValueError):                     # the morphology chain does not learn the new kinds
        from uaps_amd import morphology
        morphology(m, ok, 4)


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib
    new = {"uaps_components", "uaps_components_workspace_bytes"}
    text = open(os.path.join(ROOT, "include", "uaps_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    assert new <= declared and new <= set(_lib.SIGNATURES)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in new:
        assert hasattr(raw, n), n
    assert _lib.lib().uaps_abi_version() == 3
    body = re.search(r"typedef struct uaps_components_call \{(.*?)\} uaps_components_call;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.ComponentsCall._fields_], names
    defines = dict(re.findall(r"#define (UAPS_COMP_[A-Z_]+) (\d+)", text))
    assert {k: int(defines["UAPS_COMP_" + k.upper()]) for k in _lib.COMP_KINDS} == _lib.COMP_KINDS
    assert int(defines["UAPS_COMP_MAX_STEPS"]) == _lib.COMP_MAX_STEPS and int(defines["UAPS_COMP_MAX_CLASSES"]) == _lib.COMP_MAX_CLASSES
    assert int(defines["UAPS_COMP_ALL"]) == _lib.COMP_ALL == 2 ** 31 - 1
    assert C.sizeof(_lib.ComponentsCall) == 8 + 4 * 4 + 2 * 32 + 4 + 32 + 2 * 4 + 4 + 5 * 8    # (4 bytes of padding before the pointers)


def _call(**kw):
    from uaps_amd import _lib
    c = _lib.ComponentsCall()
    c.struct_size = C.sizeof(_lib.ComponentsCall)
    c.B, c.H, c.W, c.n_steps, c.n_classes, c.background, c.connectivity = 1, 8, 8, 1, 2, 0, 8
    c.kind[0], c.n[0] = 0, 4
    c.classes[0], c.classes[1] = 1, 2
    c.mask, c.out, c.workspace, c.workspace_bytes = 4096, 8192, 65536, 1 << 20      # never dereferenced: every call returns before a launch
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
    run = lambda c: L.uaps_components(C.byref(c))
    assert L.uaps_components(None) == EINVAL
    assert run(_call(mask=None)) == EINVAL and run(_call(out=None)) == EINVAL and run(_call(workspace=None)) == EINVAL
    assert run(_call(out=4096)) == EINVAL                                                   # out == mask
    for dim in ("B", "H", "W"):
        assert run(_call(**{dim: 0})) == EINVAL and run(_call(**{dim: -3})) == EINVAL
    assert run(_call(n_steps=0)) == EINVAL and run(_call(n_steps=9)) == EINVAL
    assert run(_call(kind=[3])) == EINVAL and run(_call(kind=[-1])) == EINVAL               # an unknown step kind
    assert run(_call(n=[0])) == EINVAL and run(_call(n=[-5])) == EINVAL                     # n < 1 of an area opening
    assert run(_call(kind=[2], n=[0])) == EINVAL                                            # ... and of a hole filling
    assert run(_call(n_steps=2, kind=[1, 0], n=[0, 0])) == EINVAL                           # ... in a later step
    assert run(_call(n_classes=0)) == EINVAL and run(_call(n_classes=9)) == EINVAL          # more than 8 classes
    assert run(_call(classes=[1, 1])) == EINVAL                                             # a duplicate
    assert run(_call(classes=[1, 0])) == EINVAL and run(_call(background=2)) == EINVAL      # a class equal to the background
    assert run(_call(connectivity=6)) == EINVAL and run(_call(connectivity=0)) == EINVAL
    assert run(_call(struct_size=C.sizeof(_lib.ComponentsCall) - 8)) == EINVAL              # a header without `stream`
    assert run(_call(H=65536, W=32768)) == ERANGE                                           # H * W = 2^31
    assert run(_call(B=64, H=2048, W=2048)) == ERANGE                                       # B * H * W * 8 = 2 GiB
    assert run(_call(B=2, H=4096, W=4096, kind=[2], n_classes=8, classes=list(range(1, 9)), workspace_bytes=1 << 40)) == ERANGE   # the workspace
    need = C.c_size_t()
    assert L.uaps_components_workspace_bytes(1, 8, 8, 1, C.byref(need)) == 0 and need.value == 2 * 256 + 512 and need.value % 256 == 0
    assert run(_call(workspace_bytes=need.value - 1)) == EWORKSPACE                         # too small
    assert run(_call(workspace=65536 + 128, workspace_bytes=1 << 20)) == EWORKSPACE         # misaligned
    holes = C.c_size_t()
    assert L.uaps_components_workspace_bytes(1, 8, 8, 2, C.byref(holes)) == 0 and holes.value == 2 * 512 + 512
    assert run(_call(kind=[2], workspace_bytes=need.value)) == EWORKSPACE                   # a hole step needs a plane per class
    assert L.uaps_components_workspace_bytes(1, 8, 8, 1, None) == EINVAL and L.uaps_components_workspace_bytes(0, 8, 8, 1, C.byref(need)) == EINVAL
    assert L.uaps_components_workspace_bytes(1, 8, 8, 0, C.byref(need)) == EINVAL and L.uaps_components_workspace_bytes(1, 8, 8, 9, C.byref(need)) == EINVAL
    assert L.uaps_components_workspace_bytes(1, 65536, 32768, 1, C.byref(need)) == ERANGE
    assert L.uaps_components_workspace_bytes(2, 4096, 4096, 8, C.byref(need)) == ERANGE
    big = C.c_size_t()
    assert L.uaps_components_workspace_bytes(2, 1024, 1024, 8, C.byref(big)) == 0 and big.value == 2 ** 21 * (8 * 8 + 8)


def test_predict_instances_with_components():
    from uaps_amd import components, inference, label_instances, morphology
    net = Stub(3, 4)
    x = _batches(net, 1)[0][0]
    steps = [("area_open", 4), ("fill_holes", None)]
    mask = inference.predict(net, x)[0]
    clean = components(mask, steps, 4)
    assert not torch.equal(clean, mask)
    conf = torch.softmax(net(x), dim=1).amax(dim=1)
    plain = inference.predict_instances(net, x)
    assert all(torch.equal(a, b) for a, b in zip(inference.predict_instances(net, x, components=None)[:3], plain[:3]))
    res, ref = inference.predict_instances(net, x, components=steps), label_instances(clean, (conf,))
    for a, b in zip(res[:3], ref[:3]):
        assert torch.equal(a, b)
    assert int(plain.count.sum()) > int(res.count.sum())
    morph = [("open", "disk", 1)]
    both = components(morphology(mask, morph, 4), steps, 4)                                  # the morphology chain runs first
    assert not torch.equal(both, clean) and not torch.equal(both, morphology(clean, morph, 4))
    res, ref = inference.predict_instances(net, x, cleanup=morph, components=steps), label_instances(both, (conf,))
    for a, b in zip(res[:3], ref[:3]):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        inference.predict_instances(net, x, components=[("area_open", 0)])
    with pytest.raises(ValueError):                     # the cleanup argument keeps its validation
        inference.predict_instances(net, x, cleanup=steps)


def test_evaluate_with_components(monkeypatch):
    from uaps_amd import components, inference, metrics, morphology
    monkeypatch.setattr(metrics, "seg_confusion_per_image", _host_confusion)
    net = Stub(3, 4)
    batches = _batches(net)
    steps = [("area_open", 4), ("fill_holes", None)]
    morph = [("open", "disk", 1), ("close", "square", 1)]
    plain = inference.evaluate(net, batches)
    assert list(plain) == ["mIoU(%)", "mDice(%)", "Accuracy(%)", "images"]                  # the dict of before
    assert inference.evaluate(net, batches, components=None) == plain
    out = inference.evaluate(net, batches, components=steps)
    both = inference.evaluate(net, batches, cleanup=morph, components=steps)
    only_morph = inference.evaluate(net, batches, cleanup=morph)
    for d in (out, both, only_morph):
        assert set(d) - set(plain) == {"mIoU_clean(%)", "mDice_clean(%)"} and all(d[k] == plain[k] for k in plain)

    def clean_scores(chain):
        miou, mdice = [], []
        with torch.no_grad():
            for x, y in batches:
                clean = chain(net(x).argmax(1))
                for b in range(len(y)):
                    cm = torch.bincount(y[b].flatten() * 4 + clean[b].flatten(), minlength=16).view(4, 4)
                    m = metrics.metrics_from_confusion(cm)
                    miou.append(m["miou"]); mdice.append(m["mdice"])
        return float(np.mean(miou) * 100), float(np.mean(mdice) * 100)

    assert (out["mIoU_clean(%)"], out["mDice_clean(%)"]) == clean_scores(lambda m: components(m, steps, 4))
    assert (both["mIoU_clean(%)"], both["mDice_clean(%)"]) == clean_scores(lambda m: components(morphology(m, morph, 4), steps, 4))
    assert len({out["mIoU_clean(%)"], both["mIoU_clean(%)"], only_morph["mIoU_clean(%)"], plain["mIoU(%)"]}) == 4
    inst = inference.evaluate(net, batches, instances={"max_instances": 4096})
    with_inst = inference.evaluate(net, batches, instances={"max_instances": 4096}, components=steps)
    assert with_inst["defects_gt"] == inst["defects_gt"] and with_inst["defects_pred"] < inst["defects_pred"]
    assert all(with_inst[k] == out[k] for k in out)
    with pytest.raises(ValueError):
        inference.evaluate(net, batches, components=[("fill_holes", 0)])
    with pytest.raises(ValueError):
        inference.evaluate(net, batches, cleanup=[("clear_border",)])
