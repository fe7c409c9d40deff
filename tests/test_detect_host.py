"""Defect detection scores without a GPU: the package's numpy restatement (uaps_amd/detection.py) against the literal reference
(tests/detect_ref.py), the hand-worked figures (tests/detect_figures.py), the refusals, evaluate(detection=...) around a stub network,
summarize over parts, and the C ABI's argument checks (they return before any launch).  Every comparison of tables is exact and
`score` is compared bit for bit."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import detect_figures as F
import detect_ref as D
from conftest import ROOT

EINVAL, ERANGE = -1, -2


def _inst(ref, n_maps=0, dev="cpu"):
    from uaps_amd import InstanceResult
    labels, count, table = ref
    return InstanceResult(torch.from_numpy(labels).to(dev), torch.from_numpy(count).to(dev), torch.from_numpy(table).to(dev), n_maps)


def _run(pred, gt, conf, num_classes, scores=None, **kw):
    from uaps_amd import detection_match, label_instances
    ip = label_instances(torch.from_numpy(pred), maps=(torch.from_numpy(conf),), max_instances=16)
    ig = label_instances(torch.from_numpy(gt), max_instances=12)
    if scores is not None:
        full = np.zeros((1, 16), dtype=scores.dtype)
        full[0, :len(scores)] = scores
        scores = torch.from_numpy(full)
    return detection_match(ip, ig, num_classes, scores=scores, **kw)


@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cpu_path_equals_the_literal_reference(shape):
    from uaps_amd import COCO_THRESHOLDS, detection_match
    assert COCO_THRESHOLDS == D.COCO == (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95)
    for name in ("noise", "blobs", "full_full", "full_empty", "empty_empty"):
        _, _, _, ref_p, ref_g = D.case(name, shape, 8)
        res = detection_match(_inst(ref_p, 1), _inst(ref_g), 4)
        assert res.pred_match.shape == (shape[0], D.MP, 10) and res.target_match.shape == (shape[0], D.MG, 10)
        assert res.counts.shape == (shape[0], 4, 12) and res.score.dtype == torch.float64 and res.t1000[0] == 500
        D.assert_tables(res, D.reference(name, shape, 8), f"{name} {shape}")
    _, _, _, ref_p, ref_g = D.case("blobs", shape, 8)
    res = detection_match(_inst(ref_p, 1), _inst(ref_g), 4, iou_thresholds=D.LOW, class_agnostic=True, max_dets=3)
    D.assert_tables(res, D.reference("blobs", shape, 8, D.LOW, True, 3), f"agnostic low {shape}")
    _, _, _, ref_p, ref_g = D.case("blobs", shape, 4)
    res = detection_match(_inst(ref_p, 1), _inst(ref_g), 4, iou_thresholds=D.T32)
    D.assert_tables(res, D.reference("blobs", shape, 4, D.T32), f"T32 {shape}")


def test_the_package_labels_and_the_reference_labels_detect_alike():
    from uaps_amd import detection_match, label_instances
    pred, gt, conf, ref_p, ref_g = D.case("blobs", (3, 37, 53), 8)
    ip = label_instances(torch.from_numpy(pred), maps=(torch.from_numpy(conf),), max_instances=D.MP)
    res = detection_match(ip, label_instances(torch.from_numpy(gt), max_instances=D.MG), 4, iou_thresholds=D.LOW)
    ref = D.reference("blobs", (3, 37, 53), 8, D.LOW)
    D.assert_tables(res, ref)
    assert ref[5][..., :6].sum() > 20 and (ref[5][..., 0] > ref[5][..., 5]).any()       # matches, and fewer of them at 1.0 than at 0.1
    D.check_summary(res.summary(), D.summary([(ref, ref_p)], [1, 2, 3], D.LOW))
    D.check_summary(res.summary(classes=[2]), D.summary([(ref, ref_p)], [2], D.LOW))


@pytest.mark.parametrize("figure", F.ALL, ids=lambda f: f.__name__)
def test_hand_worked_figures(figure):
    figure(_run)


def test_caller_scores_and_overflow():
    from uaps_amd import detection_match
    _, _, _, ref_p, ref_g = D.case("noise", (3, 37, 53), 8)
    rng = np.random.default_rng(11)
    sc = np.round(rng.standard_normal((3, D.MP)), 1)                          # many ties
    sc[0, :7] = [np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, 1e30]
    for dtype in (np.float32, np.float64):
        s = sc.astype(dtype)
        res = detection_match(_inst(ref_p), _inst(ref_g), 4, scores=torch.from_numpy(s), iou_thresholds=D.LOW)
        D.assert_tables(res, D.detect_batch(ref_p, ref_g, 4, D.LOW, scores=s), str(dtype))
    ref = D.detect_batch(ref_p, ref_g, 4, D.LOW, scores=sc)
    assert not ref[6][1:].all()                                               # noise overflows its tables: those images are skipped
    got = res.summary()
    assert got["images_skipped"] == int((~ref[6]).sum()) > 0 and got["images"] == int(ref[6].sum())
    D.check_summary(got, D.summary([(ref, ref_p)], [1, 2, 3], D.LOW))


def test_summarize_over_parts_equals_the_concatenation():
    from uaps_amd import InstanceResult, detection, detection_match
    _, _, _, ref_p, ref_g = D.case("blobs", (3, 37, 53), 8)
    whole = detection_match(_inst(ref_p, 1), _inst(ref_g), 4, iou_thresholds=D.LOW)
    cut = lambda r, sl: InstanceResult(r.labels[sl], r.count[sl], r.table[sl], r.n_maps)
    parts = [detection_match(cut(_inst(ref_p, 1), sl), cut(_inst(ref_g), sl), 4, iou_thresholds=D.LOW).sums()
             for sl in (slice(0, 1), slice(1, 3))]
    assert parts[0].rows.shape == (D.MP, 3) and parts[0].rows.dtype == torch.float64 and parts[0].n_gt.shape == (3,)
    assert detection.summarize(parts, [1, 2, 3], D.LOW, 3) == whole.summary()
    empty = detection.summarize([], [1, 2], D.COCO, 0)
    assert math.isnan(empty["mAP"]) and empty["n_gt"] == 0 and empty["images"] == 0


def test_refusals():
    from uaps_amd import InstanceResult, detection_match, label_instances
    conf = torch.full((2, 4, 4), 0.5)
    a = label_instances(torch.ones((2, 4, 4), dtype=torch.int64), maps=(conf,))
    plain = label_instances(torch.ones((2, 4, 4), dtype=torch.int64))
    assert detection_match(a, plain, 2).counts[:, 1].tolist() == [[1] * 12] * 2
    with pytest.raises(ValueError, match="map"):
        detection_match(plain, plain, 2)
    for bad in ((), (0.5, 0.5), (0.6, 0.5), (0.05,), (1.001,), (0.5005,), (float("nan"),), tuple(0.1 + 0.001 * i for i in range(33))):
        with pytest.raises(ValueError):
            detection_match(a, plain, 2, iou_thresholds=bad)
    assert detection_match(a, plain, 2, iou_thresholds=(0.1, 0.1 + 0.001 + 1e-12, 1.0)).t1000 == (100, 101, 1000)
    with pytest.raises(ValueError):
        detection_match(a, label_instances(torch.ones((2, 4, 5), dtype=torch.int64)), 2)
    with pytest.raises(ValueError):
        detection_match(a, InstanceResult(*(t.to("meta") for t in plain[:3])), 2)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            detection_match(a, plain, bad)
    with pytest.raises(TypeError):
        detection_match(a, plain.labels, 2)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            detection_match(a, plain, 2, max_dets=bad)
    with pytest.raises(TypeError):
        detection_match(a, plain, 2, scores=torch.zeros((2, 256), dtype=torch.float16))
    with pytest.raises(ValueError):
        detection_match(a, plain, 2, scores=torch.zeros((2, 255)))
    big = InstanceResult(a.labels, a.count, torch.zeros((2, 4097, 9), dtype=torch.int64), 1)
    with pytest.raises(ValueError, match="max_instances"):
        detection_match(big, plain, 2)
    with pytest.raises(ValueError):
        detection_match(a, plain, 2).summary(classes=[2])


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


def test_evaluate_with_detection_around_a_stub(monkeypatch):
    from uaps_amd import detection, detection_match, inference, label_instances, metrics
    monkeypatch.setattr(metrics, "seg_confusion_per_image", _host_confusion)
    net = Stub(3, 4)
    gen = torch.Generator().manual_seed(2)
    smooth = lambda t: torch.nn.functional.avg_pool2d(t, 5, 1, 2)
    batches = []
    for _ in range(2):
        x = smooth(torch.randn(2, 3, 24, 31, generator=gen))
        with torch.no_grad():
            y = (net(x) + 0.6 * smooth(torch.randn(2, 4, 24, 31, generator=gen))).argmax(1)
        batches.append((x, y))
    plain = inference.evaluate(net, batches)
    out = inference.evaluate(net, batches, detection=True)
    new = ["mAP(%)", "AP50(%)", "AP75(%)", "DefectAR(%)", "detection_images_skipped"]
    assert list(out) == list(plain) + new and all(out[k] == plain[k] for k in plain)

    def by_hand(thresholds=D.COCO, classes=None, max_dets=None, **lab):
        parts = []
        with torch.no_grad():
            for x, y in batches:
                logits = net(x)
                conf = torch.softmax(logits, dim=1).amax(dim=1)
                p, t = label_instances(logits.argmax(1), maps=(conf,), **lab), label_instances(y, **lab)
                parts.append(detection_match(p, t, 4, iou_thresholds=thresholds, max_dets=max_dets).sums(classes))
        return detection.summarize(parts, [1, 2, 3] if classes is None else classes, thresholds, 4)
    s = by_hand()
    assert s["n_gt"] > 0 and 0.0 < s["AP50"] <= 1.0 and out["detection_images_skipped"] == 0
    for key, name in (("mAP(%)", "mAP"), ("AP50(%)", "AP50"), ("AP75(%)", "AP75"), ("DefectAR(%)", "AR")):
        assert out[key] == 100 * s[name], key
    kw = {"iou_thresholds": (0.1, 0.3, 0.5), "min_area": 3, "connectivity": 4, "max_instances": 64, "classes": [3], "max_dets": 5}
    one = inference.evaluate(net, batches, detection=kw)
    s = by_hand((0.1, 0.3, 0.5), [3], 5, min_area=3, connectivity=4, max_instances=64)
    assert s["n_gt"] > 0 and s["mAP"] == s["mAP"]
    assert one["mAP(%)"] == 100 * s["mAP"] and one["AP50(%)"] == 100 * s["AP50"] and math.isnan(one["AP75(%)"])
    both = inference.evaluate(net, batches, instances=True, detection=True)
    assert list(both)[-5:] == new and both["mAP(%)"] == out["mAP(%)"] and "PQ(%)" in both
    few = inference.evaluate(net, batches, detection={"max_instances": 1})
    assert few["detection_images_skipped"] > 0
    assert inference.evaluate(net, batches, detection=None) == plain == inference.evaluate(net, batches, detection=False)
    with pytest.raises(TypeError):
        inference.evaluate(net, batches, detection={"iou_threshold": 0.5})
    with pytest.raises(ValueError):
        inference.evaluate(net, batches, detection={"iou_thresholds": (0.05,)})


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib
    new = {"uaps_detect_workspace_bytes", "uaps_detect_match"}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uaps_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    assert new <= declared and new <= set(_lib.SIGNATURES)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in new:
        assert hasattr(raw, n), n
    assert _lib.lib().uaps_abi_version() == 3                                 # additions only
    body = re.search(r"typedef struct uaps_detect_call \{(.*?)\} uaps_detect_call;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.DetectCall._fields_], names
    for line in ("#define UAPS_DETECT_MAX_THRESHOLDS 32", "#define UAPS_DETECT_MAX_CANDIDATES 10", "#define UAPS_DETECT_MAX_ROWS 4096"):
        assert line in hdr
    assert (_lib.DETECT_MAX_THRESHOLDS, _lib.DETECT_MAX_CANDIDATES, _lib.DETECT_MAX_ROWS) == (32, 10, 4096)
    # sizeof(uaps_detect_call): 8 x 4 bytes, 32 x 4 bytes, 6 pointers, 2 x 4 bytes, 7 pointers, pointer, size_t, pointer
    assert C.sizeof(_lib.DetectCall) == 32 + 128 + 48 + 8 + 56 + 24 and _lib.DetectCall.stream.offset == C.sizeof(_lib.DetectCall) - 8
    L = _lib.lib()
    assert L.uaps_detect_match(_call(num_classes=0)) == ERANGE
    assert L.uaps_detect_match(_call(num_classes=0, struct_size=C.sizeof(_lib.DetectCall) - 8)) == EINVAL
    assert L.uaps_detect_match(_call(num_classes=0, struct_size=C.sizeof(_lib.DetectCall) + 64)) == ERANGE      # a later header's


def _call(thresholds=(500, 750), **kw):
    from uaps_amd import _lib
    c = _lib.DetectCall()
    c.struct_size = C.sizeof(_lib.DetectCall)
    c.B, c.H, c.W, c.num_classes, c.class_agnostic, c.T, c.max_dets, c.max_pred, c.max_gt = 1, 8, 8, 4, 0, len(thresholds), 0, 16, 8
    for i, t in enumerate(thresholds):
        c.t1000[i] = t
    # never dereferenced: every call below returns before a launch
    c.pred_labels = c.target_labels = c.pred_count = c.target_count = c.pred_table = c.target_table = 4096
    c.scores = c.score = c.rank = c.pred_match = c.pred_inter = c.target_match = c.counts = c.workspace = 4096
    c.workspace_bytes = 1 << 40
    for k, v in kw.items():
        setattr(c, k, v)
    return C.byref(c)


def test_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()
    n = C.c_size_t()
    assert L.uaps_detect_workspace_bytes(16, 256, 256, 10, C.byref(n)) == 0
    rows = 16 * 256                       # the pair matrix, the lists (10 x 16 bytes a row), list lengths, keys, sequence; one word an image
    assert n.value == rows * 256 * 4 + rows * 160 + rows * 4 + rows * 8 + rows * 8 + 256 and n.value % 256 == 0
    assert L.uaps_detect_workspace_bytes(1, 1, 1, 1, C.byref(n)) == 0 and n.value == 6 * 256
    assert L.uaps_detect_workspace_bytes(1, 8, 8, 1, None) == EINVAL
    for bad in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, -1, 1)):
        assert L.uaps_detect_workspace_bytes(*bad, C.byref(n)) == EINVAL
    for bad in ((1, 8, 8, 0), (1, 8, 8, 33), (1, 4097, 8, 1), (1, 8, 4097, 1), (32, 4096, 4096, 1)):
        assert L.uaps_detect_workspace_bytes(*bad, C.byref(n)) == ERANGE, bad
    assert L.uaps_detect_workspace_bytes(31, 4096, 4096, 32, C.byref(n)) == 0
    run = L.uaps_detect_match
    assert run(None) == EINVAL
    for field in ("pred_labels", "target_labels", "pred_count", "target_count", "pred_table", "target_table", "score", "rank",
                  "pred_match", "pred_inter", "target_match", "counts", "workspace"):
        assert run(_call(**{field: None})) == EINVAL, field
    assert run(_call(struct_size=C.sizeof(_lib.DetectCall) - 8)) == EINVAL                   # a header without `stream`
    assert run(_call(struct_size=0)) == EINVAL
    assert run(_call(class_agnostic=2)) == EINVAL and run(_call(class_agnostic=-1)) == EINVAL and run(_call(max_dets=-1)) == EINVAL
    for dim in ("B", "H", "W", "max_pred", "max_gt"):
        assert run(_call(**{dim: 0})) == EINVAL, dim
    need = C.c_size_t()
    assert L.uaps_detect_workspace_bytes(1, 16, 8, 2, C.byref(need)) == 0
    assert run(_call(workspace_bytes=need.value - 1)) == EINVAL                              # too small
    assert run(_call(workspace=4096 + 128)) == EINVAL and run(_call(workspace=4096 + 4)) == EINVAL      # not 256-byte aligned
    assert run(_call(num_classes=0)) == ERANGE and run(_call(num_classes=65)) == ERANGE
    assert run(_call(H=65536, W=32768)) == ERANGE                                            # H * W = 2^31
    assert run(_call(T=0)) == ERANGE and run(_call(T=33)) == ERANGE
    for bad in ((99,), (1001,), (500, 500), (750, 500), (0,), (-500,), (100, 1000, 1000)):
        assert run(_call(thresholds=bad)) == ERANGE, bad
    assert run(_call(max_pred=4097)) == ERANGE and run(_call(max_gt=4097)) == ERANGE
    assert run(_call(B=32, max_pred=4096, max_gt=4096)) == ERANGE                            # a 2 GiB pair matrix
