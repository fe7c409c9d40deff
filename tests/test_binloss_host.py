"""The binary (one-channel sigmoid) family on the host (no GPU): the CPU path of every entry point of uaps_amd.binary_losses and the
float64 restatement of tests/binloss_ref.py against the reference-generated fixture g12_binary.npz, the new symbols, the scalar layout
and the parameter struct against the header, the argument checks of the C entry points -- each bad call returns before any HIP call,
so fake non-null device pointers are never dereferenced -- and of the Python surface, and BinaryTrainer's arguments."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import binloss_ref as R
from uaps_amd import _lib

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
P = 4096                        # a non-null "device" pointer: the calls below must refuse before touching it
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "g12_binary.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


def test_fixture_is_small_and_holds_the_cases(g):
    assert os.path.getsize(GOLD) < 100_000
    for i in range(3):
        assert g[f"c{i}_logits"].shape == (2, 1, 24, 20) and g[f"c{i}_logits"].dtype == np.float32
    assert g["c0_target"].dtype == np.uint8 and set(np.unique(g["c0_target"])) == {0, 1}
    assert g["c1_target"].dtype == np.float32 and 0 < g["c1_target"].min() and g["c1_target"].max() < 1
    assert g["c2_target"].dtype == np.uint8 and not g["c2_target"].any()
    assert "c0_bce_pw" in g.files and float(g["c0_bce_pw"]) > float(g["c0_bce"])


def test_cpu_path_of_every_entry_point_matches_the_fixture(g):
    assert R.check_fixture(g, "cpu") > 60


def test_float64_restatement_reproduces_the_fixture(g):
    """tests/binloss_ref.py is the reference of the GPU sweep: it must itself be the reference's arithmetic."""
    named = {"bce": ("bce", {}), "bce_pw": ("bce", dict(pos_weight=3.0)), "focal": ("focal", {}),
             "focal_g15": ("focal", dict(focal_alpha=0.6, focal_gamma=1.5)), "jaccard": ("jaccard", {}), "dice": ("fscore", {}),
             "dice2": ("dice2", {}), "jaccard2": ("jaccard2", {}), "tversky2": ("tversky2", dict(tversky=(0.3, 0.7)))}
    for pre, name in R.fixture_entries(g):
        if name not in named:
            continue
        term, kw = named[name]
        z = torch.tensor(g[pre + "logits"]).double().requires_grad_(True)
        t = R.fixture_target(g, pre)
        v = R.bin_terms(t.double() if t.is_floating_point() else t, z, **kw)[term]
        v.backward()
        np.testing.assert_allclose(float(v.detach()), float(g[pre + name]), rtol=2e-6, err_msg=pre + name)
        if pre + "d" + name in g.files:
            ref = g[pre + "d" + name].astype(np.float64)
            assert np.abs(z.grad.numpy() - ref).max() <= 2e-6 * np.abs(ref).max(), pre + name
    a, b = torch.tensor(g["c0_logits"]).double(), torch.tensor(g["c0_logits_b"]).double()
    np.testing.assert_allclose(float(R.sigmoid_kl(a, b)), float(g["c0_kl"]), rtol=2e-6)
    np.testing.assert_allclose(R.sigmoid_mse(a, b).numpy(), g["c0_mse_map"], rtol=1e-5, atol=1e-9)


def test_bcefocal_is_twice_the_dice_term_as_the_reference_computes_it(g):
    from uaps_amd import binary_losses as Bn
    for i in range(3):
        z, t = torch.tensor(g[f"c{i}_logits"]), R.fixture_target(g, f"c{i}_")
        np.testing.assert_allclose(float(Bn.BCEFocalLoss()(z, t)), 2 * float(Bn.DiceLoss()(z, t)), rtol=1e-6)
        np.testing.assert_allclose(float(g[f"c{i}_bce_focal"]), 2 * float(g[f"c{i}_dice"]), rtol=1e-6)


def test_thresholded_iou_and_f_score_are_the_confusion_matrix_formulas(g):
    from uaps_amd import binary_losses as Bn
    z, t = torch.tensor(g["c0_logits"]), R.fixture_target(g, "c0_")
    for thr in (0.5, 0.3):
        cm = Bn.bin_confusion(z, t, thr).numpy().astype(np.float64)
        pred = (torch.sigmoid(z.double()) > thr).numpy().reshape(-1)
        if thr == 0.5:
            want = np.bincount(2 * t.numpy().reshape(-1) + pred, minlength=4).reshape(2, 2)
            assert (cm == want).all()
        tp, fp, fn = cm[1, 1], cm[0, 1], cm[1, 0]
        np.testing.assert_allclose(float(Bn.iou(z, t, threshold=thr)), (tp + 1e-7) / (tp + fp + fn + 1e-7), rtol=1e-6)
        for beta in (1.0, 2.0):
            b2 = beta * beta
            np.testing.assert_allclose(float(Bn.f_score(z, t, beta=beta, threshold=thr)),
                                       ((1 + b2) * tp + 1e-7) / ((1 + b2) * tp + b2 * fn + fp + 1e-7), rtol=1e-6)
        m = Bn.bin_metrics_from_confusion(cm)
        np.testing.assert_allclose(m["iou"], tp / (tp + fp + fn))
        np.testing.assert_allclose(m["dice"], 2 * tp / (2 * tp + fp + fn))
        np.testing.assert_allclose(m["precision"], tp / (tp + fp))
        np.testing.assert_allclose(m["recall"], tp / (tp + fn))
        np.testing.assert_allclose(m["acc"], (cm[0, 0] + tp) / cm.sum())
    import uaps_amd
    ref = uaps_amd.metrics_from_confusion(cm)
    assert m["miou"] == ref["miou"] and m["mdice"] == ref["mdice"]              # score_validation takes the 2 x 2 matrix unchanged
    empty = Bn.bin_metrics_from_confusion(np.array([[5, 0], [0, 0]]))
    assert np.isnan(empty["iou"]) and np.isnan(empty["mdice"]) and empty["acc"] == 1.0


def test_binary_seg_loss_on_the_cpu_names_its_scalars_and_skips_bad_labels():
    from uaps_amd import binary_losses as Bn
    gen = torch.Generator().manual_seed(5)
    z = torch.randn(2, 1, 6, 8, generator=gen, requires_grad=True)
    y = torch.randint(0, 2, (2, 6, 8), generator=gen)
    y[0, 0, 0], y[1, 5, 7] = 9, -3
    crit = Bn.BinarySegLoss(R.COEFS, pos_weight=3.0, focal_gamma=1.5, beta=R.BETA, tversky=R.TVERSKY)
    assert crit.term_names == Bn.TERMS == R.TERMS
    out = crit(z, y)
    out.loss.backward()
    sc = Bn.bin_scalars(out.scalars)
    assert out.scalars.shape == (_lib.BIN_NSCALARS,) and float(sc["bad"]) == 2 and float(sc["n"]) == 2 * 6 * 8 - 2
    assert float(z.grad[0, 0, 0, 0]) == 0 and float(z.grad[1, 0, 5, 7]) == 0
    zd = z.detach().double().requires_grad_(True)
    ref = R.bin_terms(y, zd, pos_weight=3.0, focal_gamma=1.5, beta=R.BETA, tversky=R.TVERSKY)
    for k in R.TERMS + R.SUMS:
        np.testing.assert_allclose(float(sc[k]), float(ref[k].detach()), rtol=2e-5, err_msg=k)
    want = sum(R.COEFS[k] * ref[k] for k in R.TERMS)
    want.backward()
    np.testing.assert_allclose(float(out.loss.detach()), float(want.detach()), rtol=2e-5)
    assert float((z.grad.double() - zd.grad).abs().max()) <= 2e-5 * float(zd.grad.abs().max())
    # [B,1,H,W] labels, a bool mask and a float mask of zeros and ones are the same target
    a = Bn.BinarySegLoss({"bce": 1.0, "fscore": 1.0})
    y01 = (y == 1)
    v = [float(a(z.detach(), t).loss) for t in (y01.long(), y01.long().unsqueeze(1), y01, y01.float().unsqueeze(1))]
    assert max(v) - min(v) <= 1e-6 * abs(v[0])


def test_sigmoid_consistency_pair_on_the_cpu_sends_its_gradient_to_the_first_argument():
    from uaps_amd import binary_losses as Bn
    gen = torch.Generator().manual_seed(6)
    a = (torch.randn(2, 1, 5, 7, generator=gen) * 3).requires_grad_(True)
    b = (torch.randn(2, 1, 5, 7, generator=gen) * 3).requires_grad_(True)
    (Bn.sigmoid_mse_loss(a, b).sum() + Bn.sigmoid_kl_loss(a, b)).backward()
    assert b.grad is None and float(a.grad.abs().max()) > 0
    np.testing.assert_allclose(float(Bn.sigmoid_kl_loss(a, b)), float(R.sigmoid_kl(a.detach().double(), b.detach().double())), rtol=1e-5)
    with pytest.raises(AssertionError):
        Bn.sigmoid_mse_loss(a, b[:1])
    # consistency.py keeps refusing the sigmoid flag of the softmax forms
    import uaps_amd
    with pytest.raises(NotImplementedError):
        uaps_amd.softmax_mse_loss(a, b, sigmoid=True)


def test_library_exports_the_binary_symbols_and_the_abi_version_stays():
    L = _lib.lib()
    for name in ("uaps_binloss_workspace_bytes", "uaps_binloss_fwd", "uaps_binloss_bwd", "uaps_sigmoid_mse_fwd", "uaps_sigmoid_mse_bwd",
                 "uaps_sigmoid_kl_fwd", "uaps_sigmoid_kl_bwd", "uaps_bin_confusion"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    assert L.uaps_abi_version() == 3


def test_scalar_layout_and_parameter_struct_are_the_headers():
    from uaps_amd import binary_losses as Bn
    hdr = open(os.path.join(HERE, "..", "include", "uaps_hip.h")).read()
    for key, macro in (("term", "TERM"), ("loss", "LOSS"), ("bad", "BAD"), ("n", "N"), ("P", "P"), ("G", "G"), ("I", "I"), ("gP", "GP"),
                       ("gI", "GI"), ("k_bce", "KBCE"), ("k_focal", "KFOCAL"), ("nscalars", "NSCALARS")):
        m = re.search(rf"#define UAPS_BIN_S_{macro} (\d+)\s", hdr)
        assert m and int(m.group(1)) == Bn.S_OFF[key], macro
    assert Bn.S_OFF["nscalars"] == _lib.BIN_NSCALARS
    for t, name in enumerate(Bn.TERMS):
        assert f"#define UAPS_BIN_{name.upper()} {1 << t}u" in hdr, name
    assert f"#define UAPS_BIN_ALL {(1 << len(Bn.TERMS)) - 1}u" in hdr and f"#define UAPS_BIN_NTERMS {len(Bn.TERMS)}" in hdr
    assert _lib.BIN_NTERMS == len(Bn.TERMS)
    body = hdr[hdr.index("typedef struct uaps_binloss_params {"):hdr.index("} uaps_binloss_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\w+\])?\s*[,;]", body)
    assert names == [f[0] for f in _lib.BinLossParams._fields_]
    assert _lib.BinLossParams.struct_size.offset == 0 and C.sizeof(_lib.BinLossParams) == 76
    sc = Bn.bin_scalars(torch.arange(Bn.S_OFF["nscalars"], dtype=torch.float32))
    assert [float(sc[k]) for k in Bn.TERMS] == [0, 1, 2, 3, 4, 5, 6] and float(sc["I"]) == 12


def _params(terms=9, size=None, soft=0):
    p = _lib.BinLossParams()
    p.struct_size = C.sizeof(_lib.BinLossParams) if size is None else size
    p.terms, p.target_float = terms, soft
    return p


def test_binary_entry_points_refuse_bad_arguments():
    L = _lib.lib()
    n = C.c_size_t()
    assert L.uaps_binloss_workspace_bytes(2, 8, 8, C.byref(n)) == 0 and n.value > 0
    ws = n.value
    assert L.uaps_binloss_workspace_bytes(2, 8, 8, None) == EINVAL
    assert L.uaps_binloss_workspace_bytes(0, 8, 8, C.byref(n)) == EINVAL
    assert L.uaps_binloss_workspace_bytes(512, 1024, 1024, C.byref(n)) == ERANGE

    def fwd(z=P, y=P, prm="ok", B=2, H=8, W=8, s=P, w=P, wb=None):
        prm = C.byref(_params()) if prm == "ok" else prm
        return L.uaps_binloss_fwd(z, y, prm, B, H, W, s, w, ws if wb is None else wb, None)

    def bwd(z=P, y=P, prm="ok", s=P, B=2, H=8, W=8, dz=P):
        prm = C.byref(_params()) if prm == "ok" else prm
        return L.uaps_binloss_bwd(z, y, prm, s, None, B, H, W, dz, None)
    for bad in ({"z": None}, {"y": None}, {"s": None}, {"prm": None}, {"B": 0}, {"H": 0}, {"W": -2},
                {"prm": C.byref(_params(terms=0))}, {"prm": C.byref(_params(terms=128))},
                {"prm": C.byref(_params(size=C.sizeof(_lib.BinLossParams) - 4))}, {"prm": C.byref(_params(size=0))}):
        assert fwd(**bad) == EINVAL, bad
        assert bwd(**bad) == EINVAL, bad
    assert bwd(dz=None) == EINVAL
    for call in (fwd, bwd):
        assert call(B=512, H=1024, W=1024) == ERANGE                                       # 2 GiB of fp32 logits
        assert call(B=256, H=1024, W=1024) == ERANGE                                       # 2 GiB of int64 labels
    assert fwd(B=256, H=1024, W=1024, prm=C.byref(_params(soft=1)), wb=16) == EWORKSPACE      # 1 GiB of float targets is in range
    assert fwd(w=None) == EWORKSPACE and fwd(wb=16) == EWORKSPACE and fwd(wb=ws - 1) == EWORKSPACE
    # the consistency pair and the confusion matrix
    big = 1 << 29
    assert L.uaps_sigmoid_mse_fwd(None, P, 8, P, None) == EINVAL and L.uaps_sigmoid_mse_fwd(P, P, 0, P, None) == EINVAL
    assert L.uaps_sigmoid_mse_fwd(P, P, big, P, None) == ERANGE
    assert L.uaps_sigmoid_mse_bwd(P, P, None, 8, P, None) == EINVAL and L.uaps_sigmoid_mse_bwd(P, P, P, big, P, None) == ERANGE
    assert L.uaps_sigmoid_kl_fwd(P, None, 8, P, P, ws, None) == EINVAL and L.uaps_sigmoid_kl_fwd(P, P, 8, None, P, ws, None) == EINVAL
    assert L.uaps_sigmoid_kl_fwd(P, P, 8, P, None, ws, None) == EWORKSPACE and L.uaps_sigmoid_kl_fwd(P, P, 8, P, P, ws - 1, None) == EWORKSPACE
    assert L.uaps_sigmoid_kl_fwd(P, P, big, P, P, ws, None) == ERANGE
    assert L.uaps_sigmoid_kl_bwd(P, P, None, 8, None, None) == EINVAL and L.uaps_sigmoid_kl_bwd(P, P, None, -1, P, None) == EINVAL
    assert L.uaps_bin_confusion(None, P, 2, 8, 8, 0.5, P, None) == EINVAL and L.uaps_bin_confusion(P, P, 2, 8, 8, 0.5, None, None) == EINVAL
    assert L.uaps_bin_confusion(P, P, 2, 0, 8, 0.5, P, None) == EINVAL
    for thr in (0.0, 1.0, -0.1, float("nan")):
        assert L.uaps_bin_confusion(P, P, 2, 8, 8, thr, P, None) == EINVAL
    assert L.uaps_bin_confusion(P, P, 256, 1024, 1024, 0.5, P, None) == ERANGE


def test_python_surface_validates_its_arguments():
    from uaps_amd import binary_losses as Bn
    z1, z2 = torch.zeros(2, 1, 4, 4), torch.zeros(2, 2, 4, 4)
    y = torch.zeros(2, 4, 4, dtype=torch.int64)
    for call in (lambda: Bn.bce_loss(y, z2), lambda: Bn.dice_loss(y, z2), lambda: Bn.jaccard_loss(y, z2),
                 lambda: Bn.tversky_loss(y, z2, 0.5, 0.5), lambda: Bn.BinarySegLoss({"bce": 1.0})(z2, y), lambda: Bn.BCEDiceLoss()(z2, y)):
        with pytest.raises(ValueError, match="seg_losses"):                    # C != 1 points to the softmax family
            call()
    with pytest.raises(ValueError):
        Bn.BinarySegLoss({})
    with pytest.raises(ValueError):
        Bn.BinarySegLoss({"bce": 1.0, "lovasz": 1.0})
    with pytest.raises(ValueError):
        Bn.bce_loss(torch.zeros(2, 5, 4, dtype=torch.int64), z1)               # target shape
    with pytest.raises(ValueError):
        Bn.bce_loss(y, torch.zeros(2, 4, 4))                                   # logits rank
    with pytest.raises(ValueError):
        Bn.bce_loss(y, z1, pos_weight=torch.ones(2))                           # a scalar pos_weight
    with pytest.raises(TypeError):
        Bn.bce_loss(y, z1.double())
    with pytest.raises(TypeError):
        Bn.bin_confusion(z2, y)
    with pytest.raises(TypeError):
        Bn.bin_confusion(z1, y.float())
    with pytest.raises(ValueError):
        Bn.bin_confusion(z1, y, threshold=1.0)
    with pytest.raises(ValueError):
        Bn.bin_metrics_from_confusion(np.zeros((3, 3)))
    with pytest.raises(NotImplementedError):
        Bn.iou(z1, y, activation="tanh")
    assert Bn.BinarySegLoss({"fscore": .4, "bce": .6}).term_names == ("bce", "fscore")
    # the documented torch compositions: probabilities in, the per-element map, softmax2d
    p = torch.full((2, 1, 4, 4), 0.25)
    assert Bn.FocalLoss(logits=False)(p, y.unsqueeze(1).float()).dim() == 0
    assert Bn.FocalLoss(logits=True, reduce=False)(z1, y.unsqueeze(1).float()).shape == z1.shape
    assert 0 <= float(Bn.iou(z2, torch.zeros(2, 2, 4, 4), activation="softmax2d")) <= 1
    # seg_losses still refuses one channel
    from uaps_amd import seg_losses as S
    with pytest.raises(NotImplementedError):
        S.jaccard_loss(y, z1)


def test_binary_trainer_arguments():
    import uaps_amd
    from uaps_amd import binary_losses as Bn
    torch.manual_seed(3)
    tr = uaps_amd.BinaryTrainer(torch.nn.Conv2d(3, 1, 1))
    assert isinstance(tr, uaps_amd.SegTrainer) and tr.log_keys == ("loss", "bce", "fscore") and tr.threshold == 0.5
    assert tr.loss.spec.coefs == {"bce": 0.6, "fscore": 0.4} and tr.weight_keys == ()
    crit = Bn.BinarySegLoss({"focal": 1.0, "jaccard": 0.5}, focal_gamma=1.5)
    tr2 = uaps_amd.BinaryTrainer(torch.nn.Conv2d(3, 1, 1), loss=crit, threshold=0.3)
    assert tr2.loss is crit and tr2.log_keys == ("loss", "focal", "jaccard")
    base = uaps_amd.BaselineTrainer(torch.nn.Conv2d(3, 4, 1))
    assert set(tr.state_for_checkpoint(1, 0.5)) == set(base.state_for_checkpoint(1, 0.5))           # the base class's checkpoints
    with pytest.raises(TypeError):
        uaps_amd.BinaryTrainer(torch.nn.Conv2d(3, 1, 1), loss=torch.nn.BCEWithLogitsLoss())
    with pytest.raises(ValueError):
        uaps_amd.BinaryTrainer(torch.nn.Conv2d(3, 1, 1), threshold=0.0)
    # a CPU step through the torch composition: the loss falls on a fixed batch
    x, y = torch.randn(2, 3, 8, 8), (torch.rand(2, 8, 8) < 0.3).long()
    l = [float(tr.train_step(x, y)["loss"]) for _ in range(3)]
    assert l[2] < l[0] and float(tr.last["bad_labels"]) == 0
    with pytest.raises(ValueError):
        uaps_amd.BinaryTrainer(torch.nn.Conv2d(3, 2, 1)).train_step(x, y)
    val = tr.validate([(x, y)])
    assert {"miou", "mdice", "acc", "ce", "loss", "iou", "dice"} <= set(val) and np.isfinite(val["ce"])
