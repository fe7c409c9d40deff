"""Test-time augmentation without a GPU: the host function `scaled_sizes`, the CPU composition of `tta_views` / `tta_fold` /
`predict_tta` against the float64 restatement (tests/tta_ref.py), the number of forwards `predict_tta` makes, the untouched default of `inference.evaluate`, and the C ABI's
symbols and struct sizes."""
import ctypes as C
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import tta_ref as R
from conftest import ROOT

SHAPES = ((2, 4, 32, 48), (1, 8, 17, 23))


def test_scaled_sizes():
    from uaps_amd import DEFAULT_SCALES, scaled_sizes
    assert DEFAULT_SCALES == (0.5, 0.75, 1.0, 1.5, 2.0)
    for H in (17, 200, 256):
        assert scaled_sizes(H, H + 3, DEFAULT_SCALES) == [(int(H * s), int((H + 3) * s)) for s in DEFAULT_SCALES]
        assert scaled_sizes(H, H, DEFAULT_SCALES, size_multiple=1) == [(int(H * s),) * 2 for s in DEFAULT_SCALES]
    for m in (16, 8):
        assert [h for h, _ in scaled_sizes(64, 64, DEFAULT_SCALES, m)] == [32, 48, 64, 96, 128]
    sizes = scaled_sizes(200, 200, DEFAULT_SCALES, 16)
    assert all(h > 0 and h % 16 == 0 and w > 0 and w % 16 == 0 for h, w in sizes)
    assert scaled_sizes(8, 8, (0.25,), 16) == [(16, 16)]           # never below one multiple


class Stub(torch.nn.Module):
    """A seeded 1x1 convolution: a one-head "network" that runs at any size."""

    def __init__(self, cin, classes):
        super().__init__()
        torch.manual_seed(3)
        self.conv = torch.nn.Conv2d(cin, classes, 1)
        self.calls = []

    def forward(self, x):
        self.calls.append(x.shape[0])
        return 4.0 * self.conv(x)


@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_views_and_fold_against_float64(shape):
    from uaps_amd import tta_fold, tta_views
    B, Cc, H, W = shape
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, 3, H, W, generator=gen)
    for size in ((H // 2, W // 2), (H, W), (int(H * 1.5), int(W * 1.5))):
        for flip in (True, False):
            v = tta_views(x, size, flip)
            assert v.shape == ((2 if flip else 1) * B, 3) + size
            assert float((v.double() - R.views(x, size, flip)).abs().max()) <= R.TAU_VIEWS
            if flip:
                assert torch.equal(v[B:], v[:B].flip(3))
    assert torch.equal(tta_views(x, (H, W))[:B], x)
    sizes = [(int(H * s), int(W * s)) for s in R.DEFAULT_SCALES]
    for flip in (True, False):
        zs = [torch.randn((2 if flip else 1) * B, Cc, h, w, generator=gen) * 2 for h, w in sizes]
        ref = R.fold(zs, (H, W), flip)
        assert float((R.fold_gather(zs, (H, W), flip) - ref).abs().max()) < 1e-13       # the gather form IS the composition
        res = tta_fold(zs, (H, W), flip)
        views = len(zs) * (2 if flip else 1)
        assert res.probs.dtype == torch.float32 and res.mask.dtype == torch.int64
        assert float((res.probs.double() - ref).abs().max()) <= R.TAU_SUM
        assert float((res.conf.double() - ref.max(dim=1).values / views).abs().max()) <= R.TAU_SUM
        R.check_mask(res.mask, ref)
        only = tta_fold(zs, (H, W), flip, want=("mask",))
        assert only.probs is None and only.conf is None and torch.equal(only.mask, res.mask)


@pytest.mark.parametrize("shape", SHAPES)
def test_predict_tta_is_the_reference_loop(shape):
    from uaps_amd import predict_tta
    B, Cc, H, W = shape
    x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(5))
    net = Stub(3, Cc)
    sizes = [(int(H * s), int(W * s)) for s in R.DEFAULT_SCALES]
    with torch.no_grad():                   # the float64 restatement around the stub: both views of a scale, then the fold
        want = R.fold([net.eval()(R.views(x, size).float()) for size in sizes], (H, W))
    net.calls.clear()
    res = predict_tta(net, x, size_multiple=1)
    assert net.calls == [2 * B] * 5                                 # one forward of 2B images per scale
    assert not net.training
    assert float((res.probs - want).abs().max()) <= R.TAU_SUM
    assert float((res.probs.sum(1) - 10).abs().max()) <= R.TAU_SUM
    net.calls.clear()
    two = predict_tta(net, x, size_multiple=1, joined=False)
    assert net.calls == [B] * 10                                    # the reference's ten forwards
    assert float((two.probs - res.probs).abs().max()) <= R.TAU_SUM
    net.calls.clear()
    one = predict_tta(net, x, scales=(1.0,), flip=False, size_multiple=1)
    assert net.calls == [B]
    with torch.no_grad():
        assert float((one.probs - F.softmax(net(x), dim=1)).abs().max()) <= R.TAU_SUM


def test_default_size_multiple():
    from uaps_amd import ResUAPS, UNet, UNet_UAPS, tta
    assert tta.default_size_multiple(UNet(3, 4)) == 16 and tta.default_size_multiple(UNet_UAPS(3, 4, n_aux=1)) == 16
    assert tta.default_size_multiple(ResUAPS(3, 4, n_aux=0)) == 8
    assert tta.default_size_multiple(Stub(3, 4)) == 1


def test_evaluate_without_tta_is_unchanged(monkeypatch):
    """tta=None takes the path it took before: the main head's logits go to seg_confusion_per_image, predict_tta is not called."""
    import numpy as np
    from uaps_amd import inference, metrics, tta
    seen = []

    def fake_confusion(logits, labels):
        seen.append(logits)
        cm = torch.zeros(logits.shape[0], logits.shape[1], logits.shape[1], dtype=torch.int64)
        pred = logits.argmax(1)
        for b in range(logits.shape[0]):
            for t, p in zip(labels[b].flatten().tolist(), pred[b].flatten().tolist()):
                cm[b, t, p] += 1
        return cm
    monkeypatch.setattr(metrics, "seg_confusion_per_image", fake_confusion)
    monkeypatch.setattr(tta, "predict_tta", lambda *a, **k: pytest.fail("predict_tta called without tta"))
    net = Stub(3, 4)
    gen = torch.Generator().manual_seed(2)
    batches = [(torch.randn(2, 3, 16, 16, generator=gen), torch.randint(0, 4, (2, 16, 16), generator=gen)) for _ in range(2)]
    a = inference.evaluate(net, batches)
    b = inference.evaluate(net, batches, tta=None)
    assert a == b and a["images"] == 4 and np.isfinite(a["Accuracy(%)"])
    with torch.no_grad():
        assert torch.equal(seen[0], net(batches[0][0]))


def test_c_abi_symbols_and_struct_sizes(tmp_path):
    from uaps_amd import _lib
    L = _lib.lib()
    assert L.uaps_abi_version() == 3
    for name in ("uaps_tta_views", "uaps_tta_fold"):
        assert hasattr(L, name)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "uaps_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(uaps_tta_views_call), sizeof(uaps_tta_fold_call),\n'
                   '    offsetof(uaps_tta_fold_call, logits), offsetof(uaps_tta_fold_call, probs_sum), UAPS_TTA_MAX_SCALES); return 0; }\n')
    exe = tmp_path / "sizes"
    cc = os.environ.get("CC", "gcc")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(_lib.TTAViewsCall), C.sizeof(_lib.TTAFoldCall), _lib.TTAFoldCall.logits.offset,
                                     _lib.TTAFoldCall.probs_sum.offset, _lib.TTA_MAX_SCALES]
    # refusals need no device: nothing is launched
    assert L.uaps_tta_views(None) == -1 and L.uaps_tta_fold(None) == -1
    for fn, call in ((L.uaps_tta_views, _lib.TTAViewsCall()), (L.uaps_tta_fold, _lib.TTAFoldCall())):
        for size in (0, C.sizeof(call) - 8):                            # a header without `stream`
            call.struct_size = size
            assert fn(C.byref(call)) == -1
