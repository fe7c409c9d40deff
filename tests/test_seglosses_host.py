"""The supervised loss family on the host (no GPU): the float64 restatements of tests/segloss_ref.py and the CPU path of every entry
point of uaps_amd.seg_losses against the reference-generated fixture g11_seglosses.npz, the new symbols and the scalar layout, the
argument checks of the C entry points -- each bad call returns before any HIP call, so fake non-null device pointers are never
dereferenced -- and of the Python surface, and BaselineTrainer's `loss` argument."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import segloss_ref as R
from uaps_amd import _lib

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
P = 4096                        # a non-null "device" pointer: the calls below must refuse before touching it
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "g11_seglosses.npz")
# The fixture's numbers are fp32 results of the reference stored exactly; the restatement runs in float64.  Values: rtol 1e-6;
# gradients: 1e-6 of max|g| (both are a few fp32 roundings of sums over at most 960 pixels).
V_RTOL, G_TOL = 1e-6, 1e-6


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


def _case(g, pre, labels_key):
    return torch.tensor(g[pre + "logits"]), torch.tensor(g[pre + labels_key].astype(np.int64))


def _check(g, pre, name, value, grad, v_rtol=V_RTOL, g_tol=G_TOL):
    print(pre + name, float(value), float(g[pre + name]))
    np.testing.assert_allclose(float(value), float(g[pre + name]), rtol=v_rtol, err_msg=pre + name)
    if pre + "d" + name in g.files:
        ref = g[pre + "d" + name].astype(np.float64)
        err = np.abs(grad.detach().double().numpy() - ref).max()
        print(pre + "d" + name, "max err", err, "max|g|", np.abs(ref).max())
        assert err <= g_tol * np.abs(ref).max(), (pre + name, err, np.abs(ref).max())


def test_fixture_is_small_and_holds_the_three_cases(g):
    assert os.path.getsize(GOLD) < 1 << 20
    assert [tuple(g[f"c{i}_logits"].shape) for i in range(3)] == [(2, 4, 24, 20), (2, 2, 15, 13), (1, 7, 16, 16)]
    for i in range(3):
        assert g[f"c{i}_logits"].dtype == np.float32 and (g[f"c{i}_labels_ign"] == 255).any() and not (g[f"c{i}_labels"] == 255).any()
        assert len(set(g[f"c{i}_ce_w"].tolist())) > 1


def test_float64_restatement_reproduces_the_fixture(g):
    for pre, name, lab, kw in R.fixture_cases(g):
        z, y = _case(g, pre, lab)
        z = z.double().requires_grad_(True)
        v = R.seg_terms(y, z, **kw)[R.term_of(name)]
        v.backward()
        _check(g, pre, name, v.detach(), z.grad)


def test_cpu_path_of_every_entry_point_matches_the_fixture(g):
    """The CPU path computes in fp32 like the reference, in another order of operations: the bars of the restatement."""
    for pre, name, lab, _ in R.fixture_cases(g):
        z, y = _case(g, pre, lab)
        z.requires_grad_(True)
        v = R.entry_point(name, g, pre, y, z)
        assert v.dim() == 0 and v.dtype == torch.float32
        v.backward()
        _check(g, pre, name, v.detach(), z.grad)


def test_cpu_path_of_segloss_matches_the_fixture_and_names_its_scalars(g):
    from uaps_amd import seg_losses as S
    for pre, name, lab, _ in R.fixture_cases(g):
        z, y = _case(g, pre, lab)
        z.requires_grad_(True)
        out = R.seg_loss_for(name, g, pre)(z, y)
        out.loss.backward()
        _check(g, pre, name, out.loss.detach(), z.grad)
        Cc = z.shape[1]
        sc = S.seg_scalars(out.scalars, Cc)
        assert out.scalars.shape == (_lib.seg_nscalars(Cc),)
        np.testing.assert_allclose(float(sc[R.term_of(name)]), float(g[pre + name]), rtol=1e-5)
        assert float(sc["bad"]) == 0 and float(sc["n_valid"]) == float((y != 255).sum())
        np.testing.assert_allclose(float(sc["N"].sum()), float(sc["n_valid"]))
        np.testing.assert_allclose(float(sc["A"].sum()), float(sc["n_valid"]), rtol=1e-5)
    # a weighted sum of terms is the sum of the terms
    z, y = _case(g, "c0_", "labels")
    both = S.SegLoss({"jaccard": 0.25, "tversky": 2.0}, tversky=(0.3, 0.7))(z, y)
    np.testing.assert_allclose(float(both.loss), 0.25 * float(g["c0_jaccard"]) + 2.0 * float(g["c0_tversky"]), rtol=1e-5)


def test_diceloss_on_probabilities_is_the_references_form(g):
    """softmax=False takes probabilities: plain torch ops, equal to the softmax=True form on the softmax of the logits."""
    from uaps_amd import seg_losses as S
    z, y = _case(g, "c2_", "labels")
    w = [float(a) for a in g["c2_dsq_w"]]
    got = S.DiceLoss(7)(torch.softmax(z, dim=1), y.unsqueeze(1), weight=w, softmax=False)
    np.testing.assert_allclose(float(got), float(g["c2_dice_sq"]), rtol=1e-5)


def test_ignored_and_out_of_range_labels_on_the_cpu_path():
    from uaps_amd import seg_losses as S
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(2, 3, 6, 8, generator=gen, requires_grad=True)
    y = torch.randint(0, 3, (2, 6, 8), generator=gen)
    y[0, :2] = 255
    y[1, 5, 7] = 9
    crit = S.SegLoss({k: 1.0 for k in S.TERMS}, ignore_index=255)
    out = crit(z, y)
    out.loss.backward()
    sc = S.seg_scalars(out.scalars, 3)
    assert float(sc["bad"]) == 1 and float(sc["n_valid"]) == 2 * 6 * 8 - 16 - 1
    assert float(z.grad[0, :, :2].abs().max()) == 0 and float(z.grad[1, :, 5, 7].abs().max()) == 0
    zd = z.detach().double().requires_grad_(True)
    ref = sum(R.seg_terms(y, zd, ignore=255).values())
    np.testing.assert_allclose(float(out.loss.detach()), float(ref.detach()), rtol=1e-5)
    every = S.SegLoss({"ce": 1.0}, ignore_index=255)(z.detach(), torch.full((2, 6, 8), 255))
    assert bool(torch.isnan(every.loss))                                      # 0 / 0, as torch


def test_library_exports_the_segloss_symbols():
    L = _lib.lib()
    for name in ("uaps_segloss_workspace_bytes", "uaps_segloss_fwd", "uaps_segloss_bwd"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    assert L.uaps_abi_version() == 3


def test_scalar_layout_and_parameter_struct_are_the_headers():
    from uaps_amd import seg_losses as S
    hdr = open(os.path.join(HERE, "..", "include", "uaps_hip.h")).read()
    m = re.search(r"#define UAPS_SEG_S_NSCALARS\(C\) \((\d+) \+ (\d+) \* \(C\)\)", hdr)
    assert m, "UAPS_SEG_S_NSCALARS not found in the header"
    for Cc in range(2, 9):
        assert _lib.seg_nscalars(Cc) == int(m.group(1)) + int(m.group(2)) * Cc == S.s_off(Cc)["n"]
    for macro, key in (("UAPS_SEG_S_TERM 0", "term"), ("UAPS_SEG_S_LOSS 6", "loss"), ("UAPS_SEG_S_BAD 7", "bad"),
                       ("UAPS_SEG_S_NVALID 8", "n_valid"), ("UAPS_SEG_S_WSUM 9", "w_sum"), ("UAPS_SEG_S_KCE 10", "k_ce"),
                       ("UAPS_SEG_S_KFOCAL 11", "k_focal")):
        assert "#define " + macro in hdr, macro
        assert S.s_off(4)[key] == int(macro.split()[-1])
    for t, name in enumerate(S.TERMS):
        macro = "UAPS_SEG_" + name.upper()
        assert f"#define {macro} {1 << t}u" in hdr, macro
    o = S.s_off(5)
    assert [o[k] for k in ("A", "I", "N", "Z", "gA", "gI", "gZ")] == [16 + 5 * i for i in range(7)]
    # the struct: the header's fields in the header's order; 8-byte aligned int64 at the end
    body = hdr[hdr.index("typedef struct uaps_segloss_params {"):hdr.index("} uaps_segloss_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\w+\])?\s*[,;]", body)
    assert names == [f[0] for f in _lib.SegLossParams._fields_]
    assert C.sizeof(_lib.SegLossParams) == 160 and _lib.SegLossParams.ignore_index.offset == 152
    sc = S.seg_scalars(torch.arange(S.s_off(4)["n"], dtype=torch.float32), 4)
    assert [float(sc[k]) for k in S.TERMS] == [0, 1, 2, 3, 4, 5] and sc["Z"].tolist() == [28, 29, 30, 31]


def _params(terms=5, size=None):
    p = _lib.SegLossParams()
    p.struct_size = C.sizeof(_lib.SegLossParams) if size is None else size
    p.terms = terms
    return p


def test_segloss_entry_points_refuse_bad_arguments():
    L = _lib.lib()
    n = C.c_size_t()
    assert L.uaps_segloss_workspace_bytes(2, 4, 8, 8, C.byref(n)) == 0 and n.value > 0
    ws = n.value
    assert L.uaps_segloss_workspace_bytes(2, 4, 8, 8, None) == EINVAL
    assert L.uaps_segloss_workspace_bytes(0, 4, 8, 8, C.byref(n)) == EINVAL
    assert L.uaps_segloss_workspace_bytes(2, 9, 8, 8, C.byref(n)) == ERANGE

    def fwd(z=P, y=P, prm="ok", B=2, Cc=4, H=8, W=8, s=P, w=P, wb=None):
        prm = C.byref(_params()) if prm == "ok" else prm
        return L.uaps_segloss_fwd(z, y, prm, B, Cc, H, W, s, w, ws if wb is None else wb, None)

    def bwd(z=P, y=P, prm="ok", s=P, B=2, Cc=4, H=8, W=8, dz=P):
        prm = C.byref(_params()) if prm == "ok" else prm
        return L.uaps_segloss_bwd(z, y, prm, s, None, B, Cc, H, W, dz, None)
    for bad in ({"z": None}, {"y": None}, {"s": None}, {"prm": None}, {"B": 0}, {"H": 0}, {"W": -2},
                {"prm": C.byref(_params(terms=0))}, {"prm": C.byref(_params(terms=64))},
                {"prm": C.byref(_params(size=C.sizeof(_lib.SegLossParams) - 8))}, {"prm": C.byref(_params(size=0))}):
        assert fwd(**bad) == EINVAL, bad
        assert bwd(**bad) == EINVAL, bad
    assert bwd(dz=None) == EINVAL
    for call in (fwd, bwd):
        assert call(Cc=1) == ERANGE and call(Cc=9) == ERANGE
        assert call(B=64, Cc=8, H=1024, W=1024) == ERANGE                     # 2 GiB of fp32 logits
        assert call(B=256, Cc=2, H=1024, W=1024) == ERANGE                    # 2 GiB of int64 labels
    assert fwd(w=None) == EWORKSPACE and fwd(wb=16) == EWORKSPACE and fwd(wb=ws - 1) == EWORKSPACE


def test_python_surface_validates_its_arguments():
    from uaps_amd import seg_losses as S
    z1, z2, z3 = torch.zeros(2, 1, 4, 4), torch.zeros(2, 2, 4, 4), torch.zeros(2, 3, 4, 4)
    y = torch.zeros(2, 4, 4, dtype=torch.int64)
    for call in (lambda: S.ce_loss(y, z1, None), lambda: S.jaccard_loss(y, z1), lambda: S.tversky_loss(y, z1, 0.5, 0.5),
                 lambda: S.FocalLoss()(z1, y), lambda: S.DiceLoss(1)(z1, y, softmax=True), lambda: S.SegLoss({"dice": 1.0})(z1, y)):
        with pytest.raises(NotImplementedError):                               # the one-channel sigmoid branches
            call()
    assert float(S.FocalLoss(alpha=0.25)(z2, y)) > 0                           # [0.25, 0.75] on two classes
    with pytest.raises(ValueError):
        S.FocalLoss(alpha=0.25)(z3, y)                                         # a float alpha needs C = 2
    with pytest.raises(ValueError):
        S.FocalLoss(alpha=[0.1, 0.2])(z3, y)                                   # per-class list of the wrong length
    with pytest.raises(ValueError):
        S.SegLoss({"dice": 1.0, "lovasz": 1.0})
    with pytest.raises(ValueError):
        S.SegLoss({})
    with pytest.raises(ValueError):
        S.ce_loss(y, z3, [1.0, 2.0])
    with pytest.raises(ValueError):
        S.jaccard_loss(torch.zeros(2, 5, 4, dtype=torch.int64), z3)            # label shape
    with pytest.raises(ValueError):
        S.jaccard_loss(y, torch.zeros(2, 3, 4))                                # logits rank
    with pytest.raises(ValueError):
        S.jaccard_loss(y, torch.zeros(2, 9, 4, 4))                             # more classes than the kernels are built for
    with pytest.raises(ValueError):
        S.DiceLoss(4)(z3, y, softmax=True)                                     # n_classes against the channel count
    with pytest.raises(TypeError):
        S.jaccard_loss(y, z3.double())
    with pytest.raises(TypeError):
        S.jaccard_loss(y.float(), z3)
    assert S.SegLoss({"tversky": 1.0, "ce": 0.5}).term_names == ("ce", "tversky")


def test_weight_tensor_is_read_back_once_per_version():
    from uaps_amd import seg_losses as S
    w = torch.tensor([1.0, 2.0, 3.0])
    a = S._host_list(w)
    assert S._host_list(w) is a                                                # cached by identity and version
    w[0] = 5.0
    b = S._host_list(w)
    assert b is not a and b == [5.0, 2.0, 3.0]


def test_baseline_trainer_loss_argument():
    import uaps_amd
    from uaps_amd import seg_losses as S
    sig = inspect.signature(uaps_amd.BaselineTrainer.__init__)
    assert sig.parameters["loss"].default is None
    torch.manual_seed(3)
    plain = uaps_amd.BaselineTrainer(torch.nn.Conv2d(3, 4, 1))
    assert plain.loss is None and plain.log_keys == ("loss", "ce", "dice") and "log_keys" not in vars(plain)
    crit = S.SegLoss({"ce": 0.5, "tversky": 0.5}, class_weight=[1.0, 2.0, 2.0, 4.0])
    tr = uaps_amd.BaselineTrainer(torch.nn.Conv2d(3, 4, 1), loss=crit)
    assert tr.loss is crit and tr.log_keys == ("loss", "ce", "tversky")
    assert uaps_amd.BaselineTrainer.log_keys == ("loss", "ce", "dice")
    assert set(tr.state_for_checkpoint(1, 0.5)) == set(plain.state_for_checkpoint(1, 0.5))      # checkpoints are unchanged
    with pytest.raises(TypeError):
        uaps_amd.BaselineTrainer(torch.nn.Conv2d(3, 4, 1), loss=torch.nn.CrossEntropyLoss())
