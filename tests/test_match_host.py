"""Defect matching without a GPU: the package's numpy restatement (uaps_amd/matching.py) against the brute-force reference
(tests/match_ref.py), a hand-worked image, the tie, class and threshold rules, evaluate(instances=...) around a stub network, and the
C ABI's argument checks (they return before any launch).  Every comparison of tables is exact."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import instances_ref as R
import match_ref as M
from conftest import ROOT

EINVAL, ERANGE = -1, -2


def _inst(ref):
    from uaps_amd import InstanceResult
    labels, count, table = ref
    return InstanceResult(torch.from_numpy(labels), torch.from_numpy(count), torch.from_numpy(table), 0)


def _label(mask, **kw):
    from uaps_amd import label_instances
    return label_instances(torch.from_numpy(np.asarray(mask, dtype=np.int64)), **kw)


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cpu_path_equals_the_brute_force_reference(shape, connectivity):
    from uaps_amd import MATCH_COLUMNS, match_instances
    assert MATCH_COLUMNS == ("partner", "inter", "covered", "matched")
    for name in M.PATTERNS:
        _, _, _, _, ref_p, ref_g = M.case(name, shape, connectivity)
        res = match_instances(_inst(ref_p), _inst(ref_g), 4)
        assert res.pred.shape == (shape[0], M.MP, 4) and res.target.shape == (shape[0], M.MG, 4) and res.counts.shape == (shape[0], 4, 3)
        M.assert_tables(res, M.match_batch(ref_p, ref_g, 4), f"{name} {shape} c{connectivity}")
    _, _, _, _, ref_p, ref_g = M.case("noise", shape, connectivity)
    res = match_instances(_inst(ref_p), _inst(ref_g), 4, iou_threshold=0.75, class_agnostic=True)
    M.assert_tables(res, M.match_batch(ref_p, ref_g, 4, 0.75, True), f"agnostic 0.75 {shape}")


def test_the_package_labels_and_the_reference_labels_match_alike():
    """label_instances' own CPU path in front (the other tests feed scipy's tables)."""
    from uaps_amd import match_instances
    pred, gt, cp, cg, ref_p, ref_g = M.case("noise", (3, 37, 53), 8)
    res = match_instances(_label(pred, connectivity=cp, max_instances=M.MP), _label(gt, connectivity=cg, max_instances=M.MG), 4)
    M.assert_tables(res, M.match_batch(ref_p, ref_g, 4))
    assert int(res.target[..., 3].sum()) > 0 and int(res.counts[..., 0].sum()) == int(res.target[..., 3].sum()) == int(res.pred[..., 3].sum())


def test_hand_worked_image():
    from uaps_amd import match_instances
    gt = np.zeros((1, 3, 8), dtype=np.int64)
    pred = np.zeros((1, 3, 8), dtype=np.int64)
    gt[0, 0, 0:3] = 1          # A, area 3
    gt[0, 2, 0:3] = 1          # B, area 3
    pred[0, 0, 0:2] = 1        # P1 inside A: inter 2, union 3, IoU 2/3 -> matched
    pred[0, 0, 5:7] = 1        # P2: a false alarm
    pred[0, 2, 1:4] = 1        # P3, area 3, on B: inter 2, union 4, IoU exactly 1/2 -> NOT matched (strict)
    res = match_instances(_label(pred, max_instances=5), _label(gt, max_instances=4), 2)
    assert res.pred[0].tolist() == [[1, 2, 2, 1], [0, 0, 0, 0], [2, 2, 2, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert res.target[0].tolist() == [[1, 2, 2, 1], [3, 2, 2, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert res.counts[0].tolist() == [[0, 0, 0], [1, 3, 2]] and res.valid.tolist() == [True] and res.iou_threshold == 0.5
    assert res.iou()[0].tolist() == [2 / 3, 0.5, 0.0, 0.0] and res.iou().dtype == torch.float64
    assert res.sums().tolist() == [[1.0, 2.0, 1.0, 2 / 3, 2 / 3 + 2 / 3, 1.0 + 0.0 + 2 / 3, 1.0]]
    s = res.summary()
    assert s["PQ"] == pytest.approx((2 / 3) / 2.5, rel=1e-15) and s["SQ"] == pytest.approx(2 / 3, rel=1e-15) and s["RQ"] == 1 / 2.5
    assert s["precision"] == 1 / 3 and s["recall"] == 1 / 2 and s["F1"] == 2 / 5
    assert s["PRO"] == pytest.approx(2 / 3, rel=1e-15) and s["purity"] == pytest.approx(5 / 9, rel=1e-15)
    assert (s["tp"], s["fp"], s["fn"], s["n_pred"], s["n_gt"], s["images"], s["images_skipped"]) == (1, 2, 1, 3, 2, 1, 0)
    assert s["per_class"][1]["PQ"] == s["PQ"] and s["classes"] == [1]
    both = res.summary(classes=[0, 1])                        # class 0 has no defect on either side: it does not enter the mean
    assert both["PQ"] == s["PQ"] and math.isnan(both["per_class"][0]["PQ"]) and math.isnan(res.summary(classes=[0])["PQ"])
    rec = res.records()
    assert len(rec) == 1 and [r["label"] for r in rec[0]["pred"]] == [1, 2, 3] and len(rec[0]["target"]) == 2
    assert rec[0]["target"][1] == {"label": 2, "cls": 1, "area": 3, "partner": 3, "iou": 0.5, "covered": 2 / 3, "matched": False}
    assert rec[0]["pred"][0] == {"label": 1, "cls": 1, "area": 2, "partner": 1, "iou": 2 / 3, "covered": 1.0, "matched": True}
    assert rec[0]["pred"][1]["partner"] == 0 and rec[0]["pred"][1]["iou"] == 0.0
    # the half-covered pair does match nothing at any accepted threshold; the 2/3 pair stops matching above 2/3
    assert match_instances(_label(pred), _label(gt), 2, iou_threshold=0.7).counts[0, 1].tolist() == [0, 3, 2]
    with pytest.raises(ValueError):
        res.summary(classes=[2])


def test_ties_take_the_lower_number():
    from uaps_amd import match_instances
    one = np.zeros((1, 1, 5), dtype=np.int64)
    two = np.zeros((1, 1, 5), dtype=np.int64)
    one[0, 0, :] = 1                                          # one component over ...
    two[0, 0, 0:2] = 1
    two[0, 0, 3:5] = 1                                        # ... two of two pixels each
    res = match_instances(_label(one), _label(two), 2)
    assert res.pred[0, 0].tolist() == [1, 2, 4, 0] and res.target[0, :2].tolist() == [[1, 2, 2, 0], [1, 2, 2, 0]]
    res = match_instances(_label(two), _label(one), 2)
    assert res.target[0, 0].tolist() == [1, 2, 4, 0] and res.pred[0, :2].tolist() == [[1, 2, 2, 0], [1, 2, 2, 0]]


def test_class_rule():
    from uaps_amd import match_instances
    gt = np.zeros((1, 4, 6), dtype=np.int64)
    gt[0, 1:3, 1:5] = 1
    pred = gt * 2                                             # the same region, called class 2
    res = match_instances(_label(pred), _label(gt), 3)
    assert int(res.pred.abs().sum()) == 0 and int(res.target.abs().sum()) == 0
    assert res.counts[0].tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0]]
    s = res.summary()
    assert s["per_class"][1]["recall"] == 0.0 and math.isnan(s["per_class"][1]["precision"]) and s["RQ"] == 0.0 and s["PRO"] == 0.0
    assert s["precision"] == 0.0 and math.isnan(s["SQ"]) and s["purity"] == 0.0           # class 2: a false alarm; no class has a match
    res = match_instances(_label(pred), _label(gt), 3, class_agnostic=True)
    assert res.pred[0, 0].tolist() == [1, 8, 8, 1] and res.target[0, 0].tolist() == [1, 8, 8, 1]
    assert res.counts[0].tolist() == [[0, 0, 0], [1, 0, 1], [0, 1, 0]]        # tp goes to the ground truth's class
    # a class outside [0, num_classes) is matched but not counted
    assert match_instances(_label(pred), _label(gt), 2, class_agnostic=True).counts[0].tolist() == [[0, 0, 0], [1, 0, 1]]


def test_refusals():
    from uaps_amd import InstanceResult, match_instances
    a = _label(np.ones((2, 4, 4)))
    for thr in (0.49, 1.0, float("nan"), 0.0):
        with pytest.raises(ValueError):
            match_instances(a, a, 2, iou_threshold=thr)
    assert match_instances(a, a, 2, iou_threshold=0.999).counts[:, 1].tolist() == [[1, 1, 1]] * 2
    with pytest.raises(ValueError):
        match_instances(a, _label(np.ones((2, 4, 5))), 2)
    with pytest.raises(ValueError):
        match_instances(a, _label(np.ones((1, 4, 4))), 2)
    with pytest.raises(ValueError):
        match_instances(a, InstanceResult(*(t.to("meta") for t in a[:3])), 2)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            match_instances(a, a, bad)
    with pytest.raises(TypeError):
        match_instances(a, a.labels, 2)
    big = InstanceResult(a.labels, a.count, torch.zeros((2, 16384, 9), dtype=torch.int64))      # 2 * 16384^2 * 4 bytes = 2 GiB
    with pytest.raises(ValueError, match="max_instances"):
        match_instances(big, big, 2)


def test_overflow_marks_the_image_and_summary_skips_it():
    from uaps_amd import match_instances
    m = np.concatenate([R.checkerboard(9, 11), R.checkerboard(9, 11) * 0])
    m[1, 2:5, 2:5] = 1
    pred = _label(m, connectivity=4, max_instances=16)        # 50 one-pixel components in image 0
    gt = _label(m, connectivity=4, max_instances=64)
    res = match_instances(pred, gt, 2)
    assert res.valid.tolist() == [False, True]
    ref_p, ref_g = R.label_batch(m, (), 4, 0, 1, 16), R.label_batch(m, (), 4, 0, 1, 64)
    M.assert_tables(res, M.match_batch(ref_p, ref_g, 2))
    assert res.counts[0, 1].tolist() == [16, 16, 50]          # the in-table components of the overflowed image are still matched
    s = res.summary()
    assert (s["images"], s["images_skipped"], s["tp"], s["n_pred"], s["n_gt"]) == (1, 1, 1, 1, 1) and s["PQ"] == 1.0


@pytest.mark.parametrize("connectivity", (4, 8))
def test_derived_scores_equal_the_reference(connectivity):
    from uaps_amd import match_instances
    _, _, _, _, ref_p, ref_g = M.case("noise", (3, 37, 53), connectivity, 1024, 1024)
    ref = M.match_batch(ref_p, ref_g, 4)
    res = match_instances(_inst(ref_p), _inst(ref_g), 4)
    M.assert_tables(res, ref)
    assert ref[3].all() and ref[1][..., 3].sum() > 10
    M.check_scores(res, ref, ref_p, ref_g)


class Stub(torch.nn.Module):
    """A seeded 1x1 convolution: a one-head "network" that runs at any size."""

    def __init__(self, cin, classes):
        super().__init__()
        torch.manual_seed(3)
        self.conv = torch.nn.Conv2d(cin, classes, 1)

    def forward(self, x):
        return 4.0 * self.conv(x)


def _host_confusion(scored, labels):
    """The metrics kernel needs the GPU: count on the host what evaluate hands it."""
    B, Cc = scored.shape[:2]
    return torch.stack([torch.bincount(labels[b].flatten() * Cc + scored[b].argmax(0).flatten(), minlength=Cc * Cc).view(Cc, Cc)
                        for b in range(B)])


def test_evaluate_with_instances_around_a_stub(monkeypatch):
    from uaps_amd import inference, label_instances, match_instances, matching, metrics
    monkeypatch.setattr(metrics, "seg_confusion_per_image", _host_confusion)
    net = Stub(3, 4)
    gen = torch.Generator().manual_seed(2)
    smooth = lambda t: torch.nn.functional.avg_pool2d(t, 5, 1, 2)                              # blobs instead of pixel noise
    batches = []
    for _ in range(2):
        x = smooth(torch.randn(2, 3, 24, 31, generator=gen))
        with torch.no_grad():
            y = (net(x) + 0.6 * smooth(torch.randn(2, 4, 24, 31, generator=gen))).argmax(1)    # labels near the prediction
        batches.append((x, y))
    plain = inference.evaluate(net, batches)
    out = inference.evaluate(net, batches, instances=True)
    new = {"PQ(%)", "SQ(%)", "RQ(%)", "DefectPrecision(%)", "DefectRecall(%)", "PRO(%)", "defects_gt", "defects_pred", "instance_images_skipped"}
    assert list(out)[:4] == list(plain) and all(out[k] == plain[k] for k in plain) and set(out) - set(plain) == new

    def by_hand(classes=None, **kw):
        lab = {k: v for k, v in kw.items() if k != "iou_threshold"}
        rows, n_gt = [], 0
        with torch.no_grad():
            for x, y in batches:
                p, t = label_instances(net(x).argmax(1), **lab), label_instances(y, **lab)
                rows.append(match_instances(p, t, 4, iou_threshold=kw.get("iou_threshold", 0.5)).sums(classes))
                n_gt += int(t.count.sum())
        cl = [1, 2, 3] if classes is None else classes
        return matching.summarize(torch.stack(rows).sum(0).numpy(), cl, 4), n_gt
    s, n_gt = by_hand()
    assert s["tp"] > 0 and out["instance_images_skipped"] == 0
    assert out["defects_gt"] == s["n_gt"] == n_gt and out["defects_pred"] == s["n_pred"]
    for key, name in (("PQ(%)", "PQ"), ("SQ(%)", "SQ"), ("RQ(%)", "RQ"), ("DefectPrecision(%)", "precision"), ("DefectRecall(%)", "recall"),
                      ("PRO(%)", "PRO")):
        assert out[key] == pytest.approx(100 * s[name], rel=1e-12, nan_ok=True), key
    kw = {"iou_threshold": 0.6, "min_area": 3, "connectivity": 4, "max_instances": 64, "classes": [2]}
    one = inference.evaluate(net, batches, instances=kw)
    s, _ = by_hand(**kw)
    assert one["defects_gt"] == s["n_gt"] and one["PQ(%)"] == pytest.approx(100 * s["PQ"], rel=1e-12, nan_ok=True)
    assert one["defects_gt"] < out["defects_gt"]
    few = inference.evaluate(net, batches, instances={"max_instances": 1})
    assert few["instance_images_skipped"] > 0
    assert inference.evaluate(net, batches, instances=None) == plain == inference.evaluate(net, batches, instances=False)
    with pytest.raises(TypeError):
        inference.evaluate(net, batches, instances={"percentile": 95})
    with pytest.raises(TypeError):
        inference.evaluate(net, batches, instances=0.5)


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib
    new = {"uaps_match_workspace_bytes", "uaps_match_instances"}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uaps_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    assert new <= declared and new <= set(_lib.SIGNATURES)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in new:
        assert hasattr(raw, n), n
    assert _lib.lib().uaps_abi_version() == 3
    body = re.search(r"typedef struct uaps_match_call \{(.*?)\} uaps_match_call;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.MatchCall._fields_], names
    assert "#define UAPS_MATCH_MAX_CLASSES 64" in hdr and "#define UAPS_MATCH_COLUMNS 4" in hdr
    # sizeof(uaps_match_call): 6 x 4 bytes, a double, 6 pointers, 2 x 4 bytes, 3 pointers, pointer, size_t, pointer; the library reads
    # exactly that much -- a struct 8 bytes shorter is refused, this one passes the size check (and stops at the next one)
    assert C.sizeof(_lib.MatchCall) == 136 and _lib.MatchCall.stream.offset == 128
    L = _lib.lib()
    assert L.uaps_match_instances(_call(num_classes=0)) == ERANGE
    assert L.uaps_match_instances(_call(num_classes=0, struct_size=C.sizeof(_lib.MatchCall) - 8)) == EINVAL
    assert L.uaps_match_instances(_call(num_classes=0, struct_size=C.sizeof(_lib.MatchCall) + 64)) == ERANGE     # a later header's


def _call(**kw):
    from uaps_amd import _lib
    c = _lib.MatchCall()
    c.struct_size = C.sizeof(_lib.MatchCall)
    c.B, c.H, c.W, c.num_classes, c.class_agnostic, c.iou_threshold, c.max_pred, c.max_gt = 1, 8, 8, 4, 0, 0.5, 16, 8
    # never dereferenced: every call below returns before a launch
    c.pred_labels = c.target_labels = c.pred_count = c.target_count = c.pred_table = c.target_table = 4096
    c.pred_out = c.target_out = c.counts = c.workspace = 4096
    c.workspace_bytes = 1 << 40
    for k, v in kw.items():
        setattr(c, k, v)
    return C.byref(c)


def test_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()
    n = C.c_size_t()
    assert L.uaps_match_workspace_bytes(16, 256, 256, C.byref(n)) == 0 and n.value == 16 * 256 * 256 * 4
    assert L.uaps_match_workspace_bytes(1, 1, 1, C.byref(n)) == 0 and n.value == 256
    assert L.uaps_match_workspace_bytes(3, 512, 300, C.byref(n)) == 0 and n.value >= 3 * 512 * 300 * 4 and n.value % 256 == 0
    assert L.uaps_match_workspace_bytes(1, 8, 8, None) == EINVAL
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert L.uaps_match_workspace_bytes(*bad, C.byref(n)) == EINVAL
    assert L.uaps_match_workspace_bytes(2, 16384, 16384, C.byref(n)) == ERANGE               # 2 GiB exactly
    assert L.uaps_match_workspace_bytes(2, 16384, 16383, C.byref(n)) == 0
    run = L.uaps_match_instances
    assert run(None) == EINVAL
    for field in ("pred_labels", "target_labels", "pred_count", "target_count", "pred_table", "target_table", "pred_out", "target_out",
                  "counts", "workspace"):
        assert run(_call(**{field: None})) == EINVAL, field
    assert run(_call(struct_size=C.sizeof(_lib.MatchCall) - 8)) == EINVAL                    # a header without `stream`
    assert run(_call(struct_size=0)) == EINVAL
    assert run(_call(class_agnostic=2)) == EINVAL and run(_call(class_agnostic=-1)) == EINVAL
    for dim in ("B", "H", "W", "max_pred", "max_gt"):
        assert run(_call(**{dim: 0})) == EINVAL, dim
    assert run(_call(workspace_bytes=16 * 8 * 4 - 1)) == EINVAL                              # too small
    assert run(_call(workspace=4096 + 128)) == EINVAL and run(_call(workspace=4096 + 4)) == EINVAL      # not 256-byte aligned
    assert run(_call(num_classes=0)) == ERANGE and run(_call(num_classes=65)) == ERANGE
    assert run(_call(H=65536, W=32768)) == ERANGE                                            # H * W = 2^31
    for thr in (0.49, 1.0, 0.0, -1.0, float("nan"), float("inf")):
        assert run(_call(iou_threshold=thr)) == ERANGE, thr
    assert run(_call(B=2, max_pred=16384, max_gt=16384)) == ERANGE                           # a 2 GiB pair matrix
    # the Python wrapper words the last one for its caller (test_refusals)
