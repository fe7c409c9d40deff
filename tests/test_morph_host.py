"""Mask clean-up morphology without a GPU: the package's CPU restatement (uaps_amd/morphology.py, row runs on prefix sums) against
scipy (tests/morph_ref.py), the combine rule on label maps, the C ABI's argument checks (they return before any launch) and the
cleanup= keyword of inference.predict_instances / inference.evaluate around a stub network.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import morph_ref as R
from conftest import ROOT

EINVAL, ERANGE = -1, -2
SHAPES = ((1, 1), (1, 70), (70, 1), (37, 53), (64, 33))
CHECKED = (37, 53)                       # where the generator is known to give every op something to do (radii up to 5)


def _run(m, steps, num_classes=4, **kw):
    from uaps_amd import morphology
    out = morphology(torch.from_numpy(np.array(m)), steps, num_classes, **kw)
    assert out.dtype == torch.int64 and out.shape == m.shape
    return out.numpy()


@pytest.mark.parametrize("radius", (1, 2, 3, 5))
@pytest.mark.parametrize("fp", R.FOOTPRINTS)
@pytest.mark.parametrize("op", R.OPS)
def test_cpu_path_equals_scipy(op, fp, radius):
    steps = [(op, fp, radius)]
    for H, W in SHAPES:
        m = R.discs(2, H, W, 4, radius)
        ref = R.morphology(m, steps, 4)
        if (H, W) == CHECKED:
            assert R.informative(ref, m), "a vacuous case"
        assert np.array_equal(_run(m, steps), ref), (H, W)


def test_disk_and_cross_differ_from_radius_three():
    from uaps_amd.morphology import half_widths
    for r in (1, 2):
        assert half_widths("disk", r) == half_widths("cross", r) and np.array_equal(R.footprint("disk", r), R.footprint("cross", r))
    assert half_widths("disk", 3) == [3, 2, 2, 0] and half_widths("cross", 3) == [3, 2, 1, 0] and half_widths("square", 3) == [3] * 4
    for kind in R.FOOTPRINTS:
        for r in (1, 3, 8, 15):
            S, hw = R.footprint(kind, r), half_widths(kind, r)
            assert [int(S[r + d].sum() - 1) // 2 for d in range(r + 1)] == hw and np.array_equal(S, S[::-1]) and np.array_equal(S, S.T)


@pytest.mark.parametrize("steps", ([("open", "disk", 2), ("close", "square", 2)],
                                   [("erode", "cross", 1), ("dilate", "disk", 3), ("boundary", "square", 1)]), ids=("open-close", "erode-dilate-boundary"))
def test_chains(steps):
    m = R.discs(2, 37, 53, 4, 2)
    ref = R.morphology(m, steps, 4)
    assert R.informative(ref, m)
    assert np.array_equal(_run(m, steps), ref)
    one_by_one = np.array(m)
    for s in steps:
        one_by_one = _run(one_by_one, [s])
    assert np.array_equal(one_by_one, ref)


def test_class_subsets_background_and_obstacles():
    m = np.array(R.discs(2, 37, 53, 4, 2))
    m[:, 5:9, :] = 255                                   # an ignore band through discs and background
    m[:, :, 20:22] = 7                                   # a value >= num_classes
    for steps in ([("dilate", "square", 3)], [("close", "disk", 2)], [("open", "cross", 2)], [("erode", "disk", 1), ("dilate", "disk", 2)]):
        for kw in ({}, {"classes": (2,)}, {"classes": (3, 1)}, {"background": 2}, {"background": 3, "classes": (0, 1)}):
            ref = R.morphology(m, steps, 4, **kw)
            got = _run(m, steps, **kw)
            assert np.array_equal(got, ref), (steps, kw)
            # obstacles pass through and are never claimed; values the call does not select are never lost
            assert np.array_equal(got == 255, m == 255) and np.array_equal(got == 7, m == 7)
            bg = kw.get("background", 0)
            for c in range(4):
                if c != bg and c not in kw.get("classes", [k for k in range(4) if k != bg]):
                    assert np.array_equal(got == c, m == c), (steps, kw, c)
    assert (R.morphology(m, [("dilate", "square", 3)], 4) != m).any()


def test_the_lower_class_wins_a_shared_gap():
    m = np.zeros((1, 5, 9), dtype=np.int64)
    m[0, :, :3], m[0, :, 6:] = 2, 1                      # a three-pixel gap between class 2 (left) and class 1 (right)
    got = _run(m, [("dilate", "square", 2)])
    assert got[0, 2].tolist() == [2, 2, 2, 2, 1, 1, 1, 1, 1]      # column 3: only class 2 reaches; 4: both, 1 wins; 5: both
    assert np.array_equal(got, R.morphology(m, [("dilate", "square", 2)], 4))
    assert _run(m, [("dilate", "square", 2)], classes=(2,))[0, 2].tolist() == [2, 2, 2, 2, 2, 0, 1, 1, 1]


def test_opening_and_closing_properties():
    m = R.discs(2, 64, 33, 4, 2)
    for fp in R.FOOTPRINTS:
        for r in (1, 2, 3):
            opened = _run(m, [("open", fp, r)])
            assert ((opened == m) | (opened == 0)).all() and (opened != m).any()         # only original or background values
            closed = _run(m, [("close", fp, r)])
            assert (closed[m != 0] == m[m != 0]).all() and (closed != m).any()           # only background pixels change
            assert np.array_equal(_run(opened, [("open", fp, r)]), opened)               # idempotent on a binary plane's support
    edge = np.zeros((1, 9, 9), dtype=np.int64)
    edge[0, :3, :3] = 1                                                                  # a defect in the corner survives an opening
    assert np.array_equal(_run(edge, [("open", "square", 2)]), edge)


def test_argument_checks():
    from uaps_amd import morphology
    m = torch.zeros(1, 4, 4, dtype=torch.int64)
    ok = [("open", "disk", 1)]
    assert morphology(m, ok, 4) is not m
    for bad in (m.int(), m[0], m.float(), np.zeros((1, 4, 4), dtype=np.int64)):
        with pytest.raises(TypeError):
            morphology(bad, ok, 4)
    for steps in ([], ok * 9, [("melt", "disk", 1)], [("open", "hexagon", 1)], [("open", "disk", 0)], [("open", "disk", 16)],
                  [("open", "disk", 1.5)], [("open", "disk")], "open", [("open", "square", 15)] * 3):
        with pytest.raises(ValueError):
            morphology(m, steps, 4)
    for kw in ({"classes": ()}, {"classes": (1, 1)}, {"classes": (0,)}, {"classes": (4,)}, {"classes": (-1,)}, {"_band_rows": -1}):
        with pytest.raises(ValueError):
            morphology(m, ok, 4, **kw)
    with pytest.raises(ValueError):
        morphology(m, ok, 9)
    with pytest.raises(ValueError):
        morphology(torch.zeros(1, 1, 4097, dtype=torch.int64), ok, 4)


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib
    new = {"uaps_morphology", "uaps_morph_band_rows"}
    text = open(os.path.join(ROOT, "include", "uaps_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    assert new <= declared and new <= set(_lib.SIGNATURES)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in new:
        assert hasattr(raw, n), n
    assert _lib.lib().uaps_abi_version() == 3
    body = re.search(r"typedef struct uaps_morph_call \{(.*?)\} uaps_morph_call;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.MorphCall._fields_], names
    defines = dict(re.findall(r"#define (UAPS_MORPH_[A-Z_]+) (\d+)", text))
    assert {k: int(defines["UAPS_MORPH_" + k.upper()]) for k in _lib.MORPH_OPS} == _lib.MORPH_OPS
    assert {k: int(defines["UAPS_MORPH_" + k.upper()]) for k in _lib.MORPH_FOOTPRINTS} == _lib.MORPH_FOOTPRINTS
    assert int(defines["UAPS_MORPH_MAX_STEPS"]) == _lib.MORPH_MAX_STEPS and int(defines["UAPS_MORPH_MAX_CLASSES"]) == _lib.MORPH_MAX_CLASSES
    assert C.sizeof(_lib.MorphCall) == 8 + 4 * 4 + 3 * 32 + 4 + 32 + 2 * 4 + 4 + 3 * 8          # (4 bytes of padding before the pointers)


def _call(**kw):
    from uaps_amd import _lib
    c = _lib.MorphCall()
    c.struct_size = C.sizeof(_lib.MorphCall)
    c.B, c.H, c.W, c.n_steps, c.n_classes, c.background, c.band_rows = 1, 8, 8, 1, 2, 0, 0
    c.op[0], c.footprint[0], c.radius[0] = 2, 2, 1
    c.classes[0], c.classes[1] = 1, 2
    c.mask, c.out = 4096, 8192                          # never dereferenced: every call below returns before a launch
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
    run = lambda c: L.uaps_morphology(C.byref(c))
    assert L.uaps_morphology(None) == EINVAL
    assert run(_call(mask=None)) == EINVAL and run(_call(out=None)) == EINVAL
    assert run(_call(out=4096)) == EINVAL                                                   # out == mask
    for dim in ("B", "H", "W"):
        assert run(_call(**{dim: 0})) == EINVAL and run(_call(**{dim: -3})) == EINVAL
    assert run(_call(n_steps=0)) == EINVAL and run(_call(n_steps=9)) == EINVAL
    assert run(_call(op=[5])) == EINVAL and run(_call(op=[-1])) == EINVAL
    assert run(_call(footprint=[3])) == EINVAL and run(_call(footprint=[-1])) == EINVAL
    assert run(_call(n_classes=0)) == EINVAL and run(_call(n_classes=9)) == EINVAL
    assert run(_call(classes=[1, 1])) == EINVAL                                             # a duplicate
    assert run(_call(classes=[1, 0])) == EINVAL and run(_call(background=2)) == EINVAL      # a class equal to the background
    assert run(_call(band_rows=-1)) == EINVAL
    assert run(_call(struct_size=C.sizeof(_lib.MorphCall) - 8)) == EINVAL                   # a header without `stream`
    assert run(_call(radius=[0])) == ERANGE and run(_call(radius=[16])) == ERANGE
    five = dict(n_steps=5, op=[0, 1, 4, 0, 1], footprint=[0] * 5)
    assert run(_call(radius=[13] * 5, **five)) == ERANGE                                    # reach 65
    assert run(_call(n_steps=3, op=[2, 3, 0], footprint=[0] * 3, radius=[15, 15, 5])) == ERANGE     # 30 + 30 + 5
    assert run(_call(H=4097)) == ERANGE and run(_call(W=4097)) == ERANGE
    assert run(_call(B=64, H=2048, W=2048)) == ERANGE                                       # B * H * W * 8 = 2 GiB
    assert run(_call(band_rows=4096)) == ERANGE                                             # planes that cannot fit
    rows = C.c_int(-1)
    assert L.uaps_morph_band_rows(256, 256, 4, 2, C.byref(rows)) == 0 and 1 <= rows.value <= 256
    assert L.uaps_morph_band_rows(4096, 4096, 9, 64, C.byref(rows)) == 0 and rows.value >= 1        # the widest image, the longest chain
    assert L.uaps_morph_band_rows(1, 1, 2, 1, C.byref(rows)) == 0 and rows.value == 1
    assert L.uaps_morph_band_rows(8, 8, 4, 2, None) == EINVAL and L.uaps_morph_band_rows(0, 8, 4, 2, C.byref(rows)) == EINVAL
    assert L.uaps_morph_band_rows(8, 8, 1, 2, C.byref(rows)) == EINVAL and L.uaps_morph_band_rows(8, 8, 10, 2, C.byref(rows)) == EINVAL
    assert L.uaps_morph_band_rows(8, 8, 4, 0, C.byref(rows)) == EINVAL
    assert L.uaps_morph_band_rows(8, 8, 4, 65, C.byref(rows)) == ERANGE and L.uaps_morph_band_rows(8, 4097, 4, 2, C.byref(rows)) == ERANGE
    # every band the library chooses keeps its planes (the selected classes, the obstacle and free planes, two result planes per
    # class of a group of at least one) inside 64 KiB at SOME tile width of 1 .. 8 words
    for H, W, n, reach in ((256, 256, 3, 2), (1024, 1024, 3, 16), (4096, 4096, 8, 64), (130, 161, 3, 30), (5, 4096, 7, 30)):
        assert L.uaps_morph_band_rows(H, W, n + 1, reach, C.byref(rows)) == 0
        assert (n + 4) * (rows.value + 2 * reach) * 3 * 8 <= 65536 and rows.value <= H, (H, W, n, reach, rows.value)


class Stub(torch.nn.Module):
    """A 1x1 convolution per head: logits whose arg-max is speckled enough for a clean-up to matter."""

    def __init__(self, cin, classes, heads=1):
        super().__init__()
        torch.manual_seed(3)
        self.convs = torch.nn.ModuleList([torch.nn.Conv2d(cin, classes, 1) for _ in range(heads)])

    def forward(self, x):
        out = tuple(4.0 * c(x) for c in self.convs)
        return out if len(out) > 1 else out[0]


def _host_confusion(scored, labels):
    B, Cc = scored.shape[:2]
    return torch.stack([torch.bincount(labels[b].flatten() * Cc + scored[b].argmax(0).flatten(), minlength=Cc * Cc).view(Cc, Cc)
                        for b in range(B)])


def _batches(net, n=2):
    gen = torch.Generator().manual_seed(2)
    smooth = lambda v: torch.nn.functional.avg_pool2d(v, 5, 1, 2)
    out = []
    for _ in range(n):
        x = smooth(torch.randn(2, 3, 24, 31, generator=gen)) + 0.15 * torch.randn(2, 3, 24, 31, generator=gen)
        with torch.no_grad():
            y = net(smooth(x)).argmax(1)
        out.append((x, y))
    return out


def test_predict_instances_with_cleanup():
    from uaps_amd import inference, label_instances, morphology
    net = Stub(3, 4)
    x = _batches(net, 1)[0][0]
    steps = [("open", "disk", 1)]
    mask = inference.predict(net, x)[0]
    clean = morphology(mask, steps, 4)
    assert not torch.equal(clean, mask)
    conf = torch.softmax(net(x), dim=1).amax(dim=1)
    res, ref = inference.predict_instances(net, x, cleanup=steps), label_instances(clean, (conf,))
    for a, b in zip(res[:3], ref[:3]):
        assert torch.equal(a, b)
    plain = inference.predict_instances(net, x)
    assert torch.equal(plain.labels, label_instances(mask, (conf,)).labels) and int(plain.count.sum()) > int(res.count.sum())
    with pytest.raises(ValueError):
        inference.predict_instances(net, x, cleanup=[("open", "disk", 99)])


def test_evaluate_with_cleanup(monkeypatch):
    from uaps_amd import inference, metrics, morphology
    monkeypatch.setattr(metrics, "seg_confusion_per_image", _host_confusion)
    net = Stub(3, 4)
    batches = _batches(net)
    steps = [("open", "disk", 1), ("close", "square", 1)]
    plain = inference.evaluate(net, batches)
    assert list(plain) == ["mIoU(%)", "mDice(%)", "Accuracy(%)", "images"]                  # the dict of before
    assert inference.evaluate(net, batches, cleanup=None) == plain
    out = inference.evaluate(net, batches, cleanup=steps)
    assert set(out) - set(plain) == {"mIoU_clean(%)", "mDice_clean(%)"} and all(out[k] == plain[k] for k in plain)
    miou, mdice = [], []
    with torch.no_grad():
        for x, y in batches:
            clean = morphology(net(x).argmax(1), steps, 4)
            for b in range(len(y)):
                cm = torch.bincount(y[b].flatten() * 4 + clean[b].flatten(), minlength=16).view(4, 4)
                m = metrics.metrics_from_confusion(cm)
                miou.append(m["miou"]); mdice.append(m["mdice"])
    assert out["mIoU_clean(%)"] == float(np.mean(miou) * 100) and out["mDice_clean(%)"] == float(np.mean(mdice) * 100)
    assert out["mIoU_clean(%)"] != out["mIoU(%)"]
    inst = inference.evaluate(net, batches, instances={"max_instances": 4096})
    both = inference.evaluate(net, batches, instances={"max_instances": 4096}, cleanup=steps)
    assert both["defects_gt"] == inst["defects_gt"] and both["defects_pred"] < inst["defects_pred"]
    assert all(both[k] == out[k] for k in out)
    with pytest.raises(ValueError):
        inference.evaluate(net, batches, cleanup=[("open", "ring", 1)])
