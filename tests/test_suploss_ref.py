"""The references of tests/suploss_ref.py on the CPU: against torch float64 autograd of the plain formulas they restate (_cps64 of
tests/test_gpu_cps.py, _ucc64 and _cutmix_where of tests/test_gpu_ucc.py, segloss_ref.seg_terms), the comparison code of
tests/test_gpu_suploss_forms.py passing the unmutated references and rejecting every mutant, the condition that no bar swallows its
quantity on every case, the restated launch rules, and the case tables naming exactly the kernels of loss_cps.hip, loss_ucc.hip,
loss_seg.hip and loss_binary.hip that the built code object holds."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import binloss_ref as Bn
import suploss_ref as R
from test_bn_ref import kernel_pattern, norm_act_kernel_symbols

F32, F64 = np.float32, np.float64
RTOL = 1e-9                                   # float64 against float64: two orders of operations of the same formula


def _t(a, grad=False):
    return torch.from_numpy(np.asarray(a, F32).astype(F64)).requires_grad_(grad)


def _close(val, want, scale=None):
    val, want = np.asarray(val, F64), np.asarray(want.detach().numpy() if torch.is_tensor(want) else want, F64)
    assert val.shape == want.shape, (val.shape, want.shape)
    tol = RTOL * (np.abs(want).max() if scale is None else scale) + 1e-15
    assert np.abs(val - want).max() <= tol, (np.abs(val - want).max(), tol)


def _ref(cid, mut=""):
    c = R.BY_ID[cid]
    inp = R.inputs(c)
    return c, inp, R.reference(c, inp, mut)


# ---- the references against torch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["cps-c2-v4", "cps-c3-v1", "cps-c5-v4", "cps-c8-v4", "cps-sat-v4", "cps-same-v1", "cps-absent-v4", "cps-1x1"])
def test_cps_matches_torch(cid):
    from test_gpu_cps import _cps64
    c, inp, ref = _ref(cid)
    z1, z2, y = _t(inp["z1"], True), _t(inp["z2"], True), torch.from_numpy(inp["labels"])
    p1, p2 = (torch.from_numpy(np.argmax(inp[k], axis=1).astype(np.int64)) for k in ("z1", "z2"))
    from oracle import uaps_oracle as O
    if c.eps != R.EPS:                               # the restatement's Dice has the reference's eps built in
        import functools
        orig, O.dice_loss = O.dice_loss, functools.partial(O.dice_loss, eps=float(F32(c.eps)))
    try:
        ce, dice, sup, lcps, cps = _cps64(z1, z2, y, c.B_lab, p1, p2)
    finally:
        if c.eps != R.EPS:
            O.dice_loss = orig
    head = torch.stack(list(ce) + list(dice) + [sup, lcps, cps])
    _close(ref.f64["head"][0], head)
    g = (1.0, 1.0, 1.0) if c.gnull else [float(F32(x)) for x in c.g]
    (g[0] * sup + g[1] * lcps + g[2] * cps).backward()
    _close(ref.f64["dz1"][0], z1.grad)
    _close(ref.f64["dz2"][0], z2.grad)
    assert np.array_equal(ref.exact["pseudo1"], p1.numpy().astype(np.uint8)) and ref.exact["bad"] == 0


@pytest.mark.parametrize("cid", ["ucc-c2-v4", "ucc-c3-v1", "ucc-c6-v4", "ucc-c8-v1", "ucc-sat-v4", "ucc-same-v4", "ucc-one_class-v1", "ucc-1x40"])
def test_ucc_matches_torch(cid):
    from test_gpu_ucc import _ucc64
    c, inp, ref = _ref(cid)
    B = c.shape[0]
    z1, z2, y = _t(inp["z1"], True), _t(inp["z2"], True), torch.from_numpy(inp["labels"])
    p1 = torch.from_numpy(np.argmax(inp["z2"][B:2 * B], axis=1).astype(np.int64))
    p2 = torch.from_numpy(np.argmax(inp["z1"][B:2 * B], axis=1).astype(np.int64))
    r = _ucc64(z1, z2, y, B, p1, p2)
    v1, v2 = r["v1"], r["v2"]
    head = torch.stack(r["ce"] + r["dice"] + [r["sup"], r["ps"], r["ps_1"], r["ps_2"], v1.mean(), torch.exp(-v1).mean(), v2.mean(), torch.exp(-v2).mean()])
    _close(ref.f64["head"][0], head)
    for k, v in (("var1", v1), ("var2", v2)):
        if k in ref.f64:
            _close(ref.f64[k][0], v, scale=max(float(v.detach().abs().max()), 1.0))
        else:
            assert c.regime == "same" and float(v.detach().abs().max()) <= 1e-12 and not ref.exact[k].any()
    gs, gp = (1.0, 1.0) if c.gnull else (float(F32(c.g[0])), float(F32(c.g[2])))
    (gs * r["sup"] + gp * r["ps"]).backward()
    _close(ref.f64["dz1"][0], z1.grad)
    _close(ref.f64["dz2"][0], z2.grad)
    assert np.array_equal(ref.exact["pseudo1"], p1.numpy().astype(np.uint8)) and np.array_equal(ref.exact["pseudo2"], p2.numpy().astype(np.uint8))


@pytest.mark.parametrize("cid", ["seg-c5-v4", "seg-c6-v1", "seg-c6-v4", "seg-edges-v4"])
def test_seg_matches_torch(cid):
    import segloss_ref as S
    c, inp, ref = _ref(cid)
    z = _t(inp["z"], True)
    y = torch.from_numpy(R.in_range(inp["labels"], c.C)[0])
    ign = torch.from_numpy(inp["labels"] == c.ignore) if c.ignore is not None else torch.zeros(y.shape, dtype=torch.bool)
    y = torch.where((y < 0) | ign, torch.tensor(-100), y)         # every pixel that enters no term: the restatement's ignore value
    w = [float(x) for x in inp["class_weight"]]
    al, be = (float(F32(x)) for x in R.SEG_TVERSKY)
    terms = S.seg_terms(y, z, class_weight=w, ignore=-100, tversky=(al, be), eps=float(F32(c.eps)))
    coef = {k: float(F32(v)) for k, v in zip(S.TERMS, R.SEG_COEF) if v}
    loss = sum(v * terms[k] for k, v in coef.items())
    _close(ref.f64["terms"][0], torch.stack([terms[k] for k in ("ce", "dice", "jaccard", "tversky")] + [loss]))
    ((1.0 if c.gnull else float(F32(c.g[0]))) * loss).backward()
    _close(ref.f64["dz"][0], z.grad)


@pytest.mark.parametrize("cid", ["cutmix-4x6-mixed", "cutmix-6x10-column", "cutmix-37x53-full", "cutmix-16x24-off", "cutmix-1x1-full", "cutmix-b64"])
def test_cutmix_is_torch_where(cid):
    from test_gpu_ucc import _cutmix_where
    c, inp, ref = _ref(cid)
    out, y_out = _cutmix_where(*(torch.from_numpy(inp[k]) for k in ("x_l", "y_l", "x_wk", "x_st")), inp["rl"], inp["ru"])
    assert R.CR.bits_differ(ref.exact["out"], out.numpy()) == 0 and np.array_equal(ref.exact["y_out"], y_out.numpy())
    assert ref.exact["amax"] == float(out.abs().max())


# ---- the comparison code bites -----------------------------------------------------------------------------------------------------
def test_unmutated_references_pass_and_no_bar_swallows_its_quantity():
    """Every case, the two-trip ones included: the reference rounded to float32 passes its own comparison, and the largest bar of
    every compared tensor stays below 2^-10 of the tensor's largest |value|."""
    failed = {}
    for c in R.CASES:
        ref = R.reference(c, R.inputs(c))
        bad = R.compare(ref, R.as_got(ref))[1] + [f"swallowed: {s}" for s in R.swallowed(ref)]
        if bad:
            failed[c.id] = bad
    assert not failed, failed


@pytest.mark.parametrize("mut,cid", list(R.MUTANTS.items()) + R.MUTANTS_ALSO)
def test_every_mutant_is_rejected(mut, cid):
    c = R.BY_ID[cid]
    inp = R.inputs(c)
    ratios, bad = R.compare(R.reference(c, inp), R.as_got(R.reference(c, inp, mut)))
    assert bad, (mut, cid, ratios)


def test_a_wrong_count_a_wrong_byte_and_a_value_that_is_not_a_number_are_rejected():
    c, inp, ref = _ref("ucc-edges-v4")
    for key, change in (("bad", lambda g: g.__setitem__("bad", F32(g["bad"] - 1))), ("pseudo2", lambda g: g["pseudo2"].reshape(-1).__setitem__(5, 200)),
                        ("dz1", lambda g: g["dz1"].reshape(-1).__setitem__(7, np.nan)), ("reserved", lambda g: g["reserved"].__setitem__(1, 1.0))):
        got = R.as_got(ref)
        change(got)
        assert any(b.startswith(key) for b in R.compare(ref, got)[1]), key
    assert ref.exact["bad"] == inp["n_planted"] == 2 * len(R.EDGE_LABELS)


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def test_case_table_is_consistent():
    assert len(R.BY_ID) == len(R.CASES)
    by = lambda e: [c for c in R.CASES if c.entry == e]
    for e in ("cps", "ucc"):
        cs = by(e)
        for d in ("fwd", "bwd"):
            assert {(c.C, c.V(d)) for c in cs} == {(C_, v) for C_ in R.CLASSES for v in (1, 4)}, (e, d)
        assert {(c.V("fwd"), c.V("bwd")) for c in cs if c.HW % 4 == 0} == {(4, 4), (1, 1), (4, 1), (1, 4)}, e       # the forms decide separately
        forced = [c for c in cs if c.HW % 4 == 0 and c.offs]
        assert {next(iter(c.offs)) for c in forced} == {w[0] for w in R.PTR_REASONS[e]} and all(len(c.offs) == 1 for c in forced)
        assert {c.C for c in forced} == set(R.CLASSES)
        n_out = 2 if e == "cps" else 4
        for v in (1, 4):
            assert {frozenset(n for n in R.OUT4[:n_out] if c.has(n)) for c in cs if c.V("fwd") == v} == {frozenset(s) for s in R._combos(R.OUT4[:n_out])}
        assert {c.regime for c in cs} == set(R.REGIMES) and {c.shape[2:] for c in cs} >= {(1, 40), (1, 1), (5, 7), (37, 53), (16, 24)}
        assert {c.V("fwd") for c in cs if c.edges} == {1, 4} and {c.gnull for c in cs} == {True, False}
        assert any(c.trips("fwd") == 2 and c.trips("bwd") == 2 and c.V("fwd") == 1 for c in cs), e
        assert all(c.trips() == 1 for c in cs if not c.heavy)
    assert any(c.trips() == 2 and c.V() == 4 for c in by("ucc"))
    cps = by("cps")
    assert any(c.B_lab == 1 and c.shape[0] > 2 for c in cps) and any(c.B_lab == c.shape[0] - 1 and c.B_lab > 1 for c in cps)
    assert all(1 <= c.B_lab < c.shape[0] for c in cps)
    trip = R.BY_ID["cps-trip-v1"]                          # 131 769 > 512 x 256 items in either row set
    assert [s[2] for s in trip.row_sets()] == [131769, 131769] and [s[3] for s in trip.row_sets()] == [512, 512]
    cm = by("cutmix")
    assert {c.V() for c in cm if c.HW % 4 == 0 and c.shape[3] % 4 != 0} == {1, 4}                 # the row wrap, and the same maps one pixel a lane
    assert {next(iter(c.offs)) for c in cm if c.offs} == set(R.VEC_SETS[("cutmix", "fwd")]) and all(c.V() == 1 for c in cm if c.offs)
    assert any(c.Cin == 1 for c in cm) and any(c.shape[0] == R.UCC_MAX_BATCH for c in cm) and {c.hinted for c in cm} == {True, False}
    assert {c.V() for c in cm if c.trips() == 2} == {1, 4} and {c.rects for c in cm} == {"mixed", "full", "off", "empty", "column"}
    seg = by("seg")
    assert {(c.C, c.V(d)) for c in seg for d in ("fwd", "bwd")} == {(C_, v) for C_ in (5, 6) for v in (1, 4)}
    assert any(c.V("fwd") == 4 and c.V("bwd") == 1 for c in seg) and any(c.edges for c in seg) and any(c.ignore is not None for c in seg)
    for c in R.CASES:                                      # every tensor a case passes in stays below about 30 MB (cut-mix writes three of them)
        rows = {"cps": 1, "ucc": 3, "seg": 1, "cutmix": c.Cin / c.shape[1]}[c.entry]
        assert 4 * rows * np.prod(c.shape) < 31e6, c.id
    ids = {m for m in R.MUTANTS} | {m for m, _ in R.MUTANTS_ALSO}
    assert ids == {"own_argmax", "unl_in_gt", "tie_high", "no_eps", "no_projection", "inv_n_other", "ce_on_minus1", "var_swapped", "pseudo1_from_z1",
                   "no_exp", "k_sign", "neighbour_back", "end_inclusive", "labels_not_mixed", "paste_raw"}


def test_label_edge_inputs_hold_every_planted_value():
    for cid in ("cps-edges-v4", "ucc-edges-v1", "seg-edges-v1"):
        c = R.BY_ID[cid]
        y = R.inputs(c)["labels"]
        assert set(R.edge_labels(c.C).tolist()) <= set(y.reshape(-1).tolist()), cid
    narrowed = R.edge_labels(4).astype(np.int32)             # what a narrowing to int makes of them: three become classes 1, 1 and 0
    assert narrowed.tolist() == [-1, 4, 255, -2 ** 31, 1, 1, 0, -1]


def test_grid_rule_and_trip_counts_match_the_launchers():
    assert R.grid_for(0, 512) == 1 and R.grid_for(256, 512) == 1 and R.grid_for(257, 512) == 2 and R.grid_for(131769, 512) == 512
    assert R.trips(131072, 512) == 1 and R.trips(131073, 512) == 2 and R.trips(262144, 1024) == 1 and R.trips(263169, 1024) == 2
    assert R.trips(1026 * 1024 // 4, 1024) == 2 and R.trips(2 * 725 * 725, 4096) == 2 and R.trips(2 * 3 * 840 * 840 // 4, 4096) == 2
    assert R.n_adds(100, 512, 1) >= 9 and R.n_adds(131769, 512, 1) >= 10 and R.n_adds(1026 * 256, 1024, 4) >= 16


def _lib_or_skip():
    from uaps_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libuaps_hip.so is not built")
    return _lib


def test_workspace_bytes_match_the_library():
    L = _lib_or_skip().lib()
    n = C.c_size_t()
    for c in R.CASES:
        N, Cc, H, W = c.shape
        if c.entry == "cps":
            assert L.uaps_cps_workspace_bytes(N, c.B_lab, Cc, H, W, C.byref(n)) == 0
        elif c.entry == "ucc":
            assert L.uaps_ucc_workspace_bytes(N, Cc, H, W, C.byref(n)) == 0
        elif c.entry == "seg":
            assert L.uaps_segloss_workspace_bytes(N, Cc, H, W, C.byref(n)) == 0
        else:
            continue
        assert n.value == c.workspace_bytes, (c.id, n.value)
    assert (R.workspace_bytes("cps"), R.workspace_bytes("ucc"), R.workspace_bytes("seg")) == (327680, 409600, 163840)


def test_cases_cover_every_kernel_and_name_none_that_does_not_exist():
    """The code object is the authority: the cases of this file, the seg sweep of tests/test_gpu_seglosses.py and the binary table
    name every kernel of the four sources it holds, and nothing else."""
    lib = _lib_or_skip()
    built = norm_act_kernel_symbols(lib.LIB_PATH, kernel_pattern(R.KERNEL_NAMES))
    named = set().union(*(c.kernels for c in R.CASES)) | R.seg_sweep_kernels()
    assert named == built, ("no case reaches", sorted(built - named), "no such kernel", sorted(named - built))
    per = {f: sum(k.startswith(f) for k in built) for f in ("cps_", "ucc_", "seg_")}
    assert per == {"cps_": 35, "ucc_": 37, "seg_": 35}, per
    own = set().union(*(c.kernels for c in R.CASES))
    assert {k for k in built if k.startswith(("cps_", "ucc_"))} <= own                      # CPS and UCC: by this file's cases alone
    assert {k for k in built if re.match(r"seg_\w+<[56]", k)} <= own
    built_bin = norm_act_kernel_symbols(lib.LIB_PATH, kernel_pattern(Bn.KERNEL_NAMES))
    named_bin = set().union(*(c.kernels for c in Bn.CASES)) | Bn.PAIR_KERNELS | Bn.CONFUSION_KERNELS
    assert named_bin == built_bin and len(built_bin) == 12, (sorted(built_bin - named_bin), sorted(named_bin - built_bin))


def test_every_kernel_of_the_four_sources_is_in_the_filters():
    GLOBAL = r"__global__(?:\s+__launch_bounds__\([^)]*\))?\s+void\s+(\w+)\s*\("
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uaps_amd", "csrc")
    found = lambda *fs: set().union(*(set(re.findall(GLOBAL, open(os.path.join(src, f)).read())) for f in fs))
    assert found("loss_cps.hip", "loss_ucc.hip", "loss_seg.hip") == set(R.KERNEL_NAMES)
    assert found("loss_binary.hip") == set(Bn.KERNEL_NAMES)
