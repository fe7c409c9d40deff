"""inference.evaluate composes its score families: one call with every family on returns, for each family, exactly the values of the
call with that family alone (under the same clean-up chains), in the documented key order, on the plain, the tta and the tiled path.

The fixture needs no golden file: a stub network whose "images" carry its logits.  Channels 0..2 are the main head's three-class logits,
the winner at 20 + k (k = 0..3) over zeros; channel 3 is a flag.  The auxiliary head is a quarter of the main head, with the classes
rotated by one where the flag is set.  Everything is constant on 4 x 4 blocks.  Chosen so that a GPU run and a CPU run see the same
integers (see test_gpu_composition_and_the_cpu_run)."""
import math

import numpy as np
import pytest
import torch

CLASSES, SIDE, BLOCK = 3, 32, 4
CLEANUP = [("open", "square", 1)]
COMPONENTS = [("area_open", 20), ("fill_holes", None)]
FAMILIES = {"surface": {"tolerance": 2.0}, "instances": {"max_instances": 128}, "curves": {"uncertainty": True}}
BASE_KEYS = ["mIoU(%)", "mDice(%)", "Accuracy(%)", "images"]
CLEAN_KEYS = ["mIoU_clean(%)", "mDice_clean(%)"]
FAMILY_KEYS = {"surface": ["HD95(px)", "ASSD(px)", "NSD(%)", "surface_pairs"],
               "instances": ["PQ(%)", "SQ(%)", "RQ(%)", "DefectPrecision(%)", "DefectRecall(%)", "PRO(%)", "defects_gt", "defects_pred",
                             "instance_images_skipped"],
               "curves": ["AUROC(%)", "AP(%)", "AUPRO(%)", "ECE(%)", "curve_images_skipped"]}
UNC_KEYS = ["UncAUROC(%)", "AURC"]
PATHS = {"plain": {}, "tta": {"tta": (1.0, 0.5)}, "tiled": {"tiled": {"tile": 16, "overlap": 4}}}
INTEGER_KEYS = ("images", "surface_pairs", "defects_gt", "defects_pred", "instance_images_skipped", "curve_images_skipped")
CURVE_FLOATS = ("AUROC(%)", "AP(%)", "AUPRO(%)", "ECE(%)")


class Stub(torch.nn.Module):
    """(main, aux) read off the input, at any size: main = channels 0..2, aux = main / 4 with the classes rotated where channel 3 is 1.
    Products with 0, 1 and 1/4 and sums with 0: exact in fp32 wherever they run."""

    def forward(self, x):
        main, flag = x[:, :CLASSES], x[:, CLASSES:]
        return main.contiguous(), 0.25 * (main * (1.0 - flag) + main.roll(1, 1) * flag)


def _blocks(v):
    return v.repeat_interleave(BLOCK, -2).repeat_interleave(BLOCK, -1)


def _batches(device="cpu"):
    """Two batches of two 32 x 32 "images" [2,4,32,32] with int64 labels: the main head's winner, moved to the next class on a fifth
    of the blocks; the auxiliary head disagrees on most of those and on a tenth of the others."""
    gen = torch.Generator().manual_seed(11)
    n = SIDE // BLOCK
    out = []
    for _ in range(2):
        win = torch.randint(0, CLASSES, (2, n, n), generator=gen)
        level = 20.0 + torch.randint(0, 4, (2, n, n), generator=gen)
        wrong = torch.rand(2, n, n, generator=gen) < 0.2
        flag = torch.rand(2, n, n, generator=gen) < torch.where(wrong, 0.7, 0.1)
        main = torch.nn.functional.one_hot(win, CLASSES).permute(0, 3, 1, 2) * level[:, None]
        x = _blocks(torch.cat([main, flag[:, None].float()], dim=1)).contiguous()
        y = _blocks(torch.where(wrong, (win + 1) % CLASSES, win)).contiguous()
        out.append((x.to(device), y.to(device)))
    return out


def _host_confusion(scored, labels):
    B, Cc = scored.shape[:2]
    return torch.stack([torch.bincount(labels[b].flatten() * Cc + scored[b].argmax(0).flatten(), minlength=Cc * Cc).view(Cc, Cc)
                        for b in range(B)])


def _host_uncertainty(main, aux):
    """consistency.uncertainty_map needs the GPU: sum_c KLDivLoss('none')(log_softmax(main), softmax(aux))."""
    q = torch.softmax(aux, dim=1)
    return (q * (torch.log(q) - torch.log_softmax(main, dim=1))).sum(dim=1)


@pytest.fixture
def host(monkeypatch):
    """The two ops of evaluate that exist on the GPU alone, restated for CPU tensors."""
    from uaps_amd import consistency, metrics
    monkeypatch.setattr(metrics, "seg_confusion_per_image", _host_confusion)
    monkeypatch.setattr(consistency, "uncertainty_map", _host_uncertainty)


def _families(path):
    """The family keywords of one path: the uncertainty rows exist on the plain path alone."""
    fam = dict(FAMILIES)
    if path != "plain":
        fam["curves"] = True
    return fam


def _keys(path):
    return BASE_KEYS + CLEAN_KEYS + sum(FAMILY_KEYS.values(), []) + (UNC_KEYS if path == "plain" else [])


def _same(a, b, keys):
    assert [k for k in a if k in keys] == [k for k in b if k in keys] == list(keys)
    for k in keys:
        assert repr(a[k]) == repr(b[k]), (k, a[k], b[k])


def _check_composition(net, batches, path):
    """evaluate with every family on, checked against the calls with one family each; returns the former."""
    from uaps_amd import inference
    chains = dict(cleanup=CLEANUP, components=COMPONENTS, **PATHS[path])
    fam = _families(path)
    both = inference.evaluate(net, batches, **chains, **fam)
    assert list(both) == _keys(path)
    assert both["images"] == 4 and both["surface_pairs"] > 0 and both["defects_gt"] > 0 and both["defects_pred"] > 0
    assert not any(math.isnan(v) for v in both.values())
    _same(both, inference.evaluate(net, batches, **chains), BASE_KEYS + CLEAN_KEYS)
    for name, value in fam.items():
        alone = inference.evaluate(net, batches, **chains, **{name: value})
        keys = FAMILY_KEYS[name] + (UNC_KEYS if name == "curves" and path == "plain" else [])
        assert list(alone) == BASE_KEYS + CLEAN_KEYS + keys
        _same(both, alone, BASE_KEYS + CLEAN_KEYS + keys)
    return both


@pytest.mark.parametrize("path", list(PATHS))
def test_every_family_composes(host, path):
    both = _check_composition(Stub(), _batches(), path)
    assert both["mIoU_clean(%)"] != both["mIoU(%)"] and 50.0 < both["AUROC(%)"] <= 100.0
    if path == "plain":
        assert 50.0 < both["UncAUROC(%)"] <= 100.0 and 0.0 < both["AURC"] < 1.0


def test_the_fixture_keeps_clear_of_ties_and_bin_edges():
    """What lets the GPU case compare with the CPU run: no two classes tie, the main head's softmax saturates (margins of at least 20:
    1 + 2 exp(-20) rounds to 1 in fp32, so the probabilities are 1 and about 2e-9 whoever forms the exponential), and the uncertainty
    values -- a handful of distinct numbers -- lie away from the edges of the 1024 bins over [0, 1] by far more than a rounding error."""
    net = Stub()
    for x, y in _batches():
        main, aux = net(x)
        for z in (main, aux):
            top = z.topk(2, dim=1).values
            assert float((top[:, 0] - top[:, 1]).min()) >= 5.0
        assert float((main.topk(2, dim=1).values[:, 0] - main.topk(2, dim=1).values[:, 1]).min()) >= 20.0
        assert torch.equal(torch.softmax(main, dim=1).amax(dim=1), torch.ones(y.shape))
        u = torch.unique(_host_uncertainty(main.double(), aux.double()))
        inside = u[u < 1.0] * 1024.0
        assert 0 < len(inside) <= 16 and len(u) > len(inside)                  # some pixels beyond hi = 1: the last bin, by clamping
        assert float((inside - inside.round()).abs().min()) > 1e-2
        assert float(u[u >= 1.0].min()) > 1.01


def test_off_values(host):
    from uaps_amd import inference
    net, batches = Stub(), _batches()
    plain = inference.evaluate(net, batches)
    assert list(plain) == BASE_KEYS
    # every falsy value, {} included, switches surface, instances, tiled and tta off
    for off in ({"surface": {}}, {"instances": {}}, {"tiled": {}}, {"tta": ()}, {"tta": False}, {"surface": False, "instances": None},
                {"curves": None}, {"curves": False}, {"tiled": {}, "tta": 0, "surface": 0, "instances": ()}):
        assert repr(inference.evaluate(net, batches, **off)) == repr(plain), off
    # curves is off for None and False alone: an empty dict asks for the defaults
    on = inference.evaluate(net, batches, curves={})
    assert list(on) == BASE_KEYS + FAMILY_KEYS["curves"] and repr(on) == repr(inference.evaluate(net, batches, curves=True))
    # tiled={} is off, so the uncertainty rows are not refused beside it
    assert list(inference.evaluate(net, batches, curves={"uncertainty": True}, tiled={}, tta=()))[-2:] == UNC_KEYS


def test_validation_order(host):
    """Before the first batch is read: cleanup, components, curves, tiled (with its refusal of tta), surface, instances."""
    from uaps_amd import inference

    def batches():
        pytest.fail("a batch was read before the arguments were checked")
        yield

    bad = [("cleanup", [("clear_border",)], ValueError, "morphology"), ("components", [("area_open", 0)], ValueError, "components"),
           ("curves", {"percentile": 95}, TypeError, "curves is True or a dict"), ("tiled", 3, TypeError, "tiled is True or a dict"),
           ("surface", {"bins": 4}, TypeError, "surface is True or a dict"), ("instances", {"bins": 4}, TypeError, "instances is True or a dict")]
    for i, (_, _, exc, text) in enumerate(bad):
        with pytest.raises(exc, match=text):
            inference.evaluate(Stub(), batches(), **{name: value for name, value, _, _ in bad[i:]})
    with pytest.raises(ValueError, match="tiled together with tta"):
        inference.evaluate(Stub(), batches(), tiled=True, tta=True, surface={"bins": 4})
    with pytest.raises(ValueError, match="uncertainty=True"):
        inference.evaluate(Stub(), batches(), curves={"uncertainty": True}, tiled=3)


def test_empty_batches(host):
    from uaps_amd import inference
    with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):                 # numpy's mean of nothing
        out = inference.evaluate(Stub(), [], cleanup=CLEANUP, components=COMPONENTS, **FAMILIES)
    assert list(out) == _keys("plain")
    zero = {k: out[k] for k in INTEGER_KEYS}
    assert zero == dict.fromkeys(INTEGER_KEYS, 0) and all(type(v) is int for v in zero.values())
    assert all(math.isnan(out[k]) for k in out if k not in INTEGER_KEYS)
    with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):
        out = inference.evaluate(Stub(), [], instances={"classes": [1, 2]}, tta=True)
    assert out["defects_gt"] == out["defects_pred"] == out["instance_images_skipped"] == 0 and math.isnan(out["PQ(%)"])


@pytest.mark.gpu
def test_gpu_composition_and_the_cpu_run(monkeypatch):
    """The same property on the device, and the device against the CPU path.  The integer-valued keys are equal on all three paths.
    The float keys are held to the tolerances of the evaluate tests of test_gpu_surface.py (HD95: rel 1e-9) and test_gpu_curves.py
    (every other key: rel 1e-12): all of them on the plain path, where the fixture makes every table an integer both sides agree on
    (test_the_fixture_keeps_clear_of_ties_and_bin_edges); under tta and tiled all but the four curve scores, because there the scored
    probabilities pass through the kernels' bilinear mix and window blend, which the CPU composition matches to fp32 rounding only --
    enough for the arg-max masks everything else is computed from, not for bin counts and fixed-point sums."""
    dev = torch.device("cuda:0")
    net = Stub().to(dev)
    on_device = {path: _check_composition(net, _batches(dev), path) for path in PATHS}
    from uaps_amd import consistency, metrics
    monkeypatch.setattr(metrics, "seg_confusion_per_image", _host_confusion)
    monkeypatch.setattr(consistency, "uncertainty_map", _host_uncertainty)
    from uaps_amd import inference
    for path, got in on_device.items():
        ref = inference.evaluate(Stub(), _batches(), cleanup=CLEANUP, components=COMPONENTS, **PATHS[path], **_families(path))
        assert list(got) == list(ref)
        for k in got:
            print(path, k, got[k], ref[k])
        for k in got:
            if k in INTEGER_KEYS:
                assert got[k] == ref[k] and type(got[k]) is int, (path, k)
            elif path == "plain" or k not in CURVE_FLOATS:
                assert got[k] == pytest.approx(ref[k], rel=1e-9 if k == "HD95(px)" else 1e-12, nan_ok=True), (path, k)
