"""The references of tests/strided_ref.py on the CPU: every reference against torch in float64 (F.conv2d and its autograd,
F.max_pool2d(return_indices=True), slicing), the comparisons of tests/test_gpu_strided_forms.py passing the unmutated references and
rejecting every mutant, the restated weight-gradient plan against uaps_convs_wrw_workspace_bytes, and the case table naming exactly the
kernels of uaps_amd/csrc/conv_strided.hip that the built code object holds."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import strided_ref as R
from test_bn_ref import kernel_pattern, norm_act_kernel_symbols

F32 = np.float32
CONV_IDS = [c.id for c in R.CONV]


# ---- the references against torch float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CONV_IDS)
def test_conv_references_match_torch(cid):
    c = R.BY_ID[cid]
    inp = R.conv_inputs(c, "real")
    x = torch.from_numpy(inp["x"].astype(np.float64)).requires_grad_(True)
    w = torch.from_numpy(inp["w"].astype(np.float64)).requires_grad_(True)
    y = F.conv2d(x, w, None, c.s, c.p)
    assert tuple(y.shape) == (c.B, c.Cout, c.OH, c.OW)
    y.backward(torch.from_numpy(inp["dy"].astype(np.float64)))
    tol = 1e-12 * max(R.contraction(c, op) for op in ("fwd", "dx", "dw"))
    assert np.abs(R.conv_fwd(inp["x"], inp["w"], c.s, c.p) - y.detach().numpy()).max() <= tol
    dx = R.conv_dx(inp["dy"], inp["w"], c.s, c.p, c.H, c.W)
    assert np.abs(dx - x.grad.numpy()).max() <= tol
    assert np.abs(dx - R.conv_dx_adjoint(inp["dy"], inp["w"], c.s, c.p, c.H, c.W)).max() <= tol
    assert np.abs(R.conv_dw(inp["dy"], inp["x"], c.ks, c.s, c.p) - w.grad.numpy()).max() <= tol


def test_contraction_lengths_and_magnitudes():
    """K (the reference run on ones) counts the valid taps x channels: the full ks^2 C inside, fewer at the border, none where padding
    alone is read; sum|terms| is the reference run on the absolute values."""
    c = R.BY_ID["c3s1-nw1"]
    inp = R.conv_inputs(c, "real")
    val, K, mag = R.conv_reference(c, inp, "fwd")
    assert K.max() == 9 * c.Cin == R.contraction(c, "fwd") and K[0, 0, 0, 0] == 4 * c.Cin and np.all(mag >= np.abs(val))
    val, K, mag = R.conv_reference(c, inp, "dw")
    assert K.max() == c.B * c.OH * c.OW == R.contraction(c, "dw") and K[0, 0, 0, 0] == (c.OH - 1) * (c.OW - 1)
    c = R.BY_ID["c1s1-p1"]
    val, K, mag = R.conv_reference(c, R.conv_inputs(c, "real"), "fwd")
    assert np.all(K[:, :, 0] == 0) and np.all(val[:, :, :, -1] == 0) and K.max() == c.Cin


def test_packed_layouts():
    w = np.arange(2 * 3 * 9, dtype=F32).reshape(2, 3, 3, 3) + 1
    wf, wb = R.pack_weights(w)
    assert wf.shape == (9 * 4 * 16,) and wb.shape == (9 * 4 * 16,)
    wf, wb = wf.reshape(9, 4, 16), wb.reshape(9, 4, 16)
    assert wf[5, 2, 1] == w[1, 2, 1, 2] and wb[5, 1, 2] == w[1, 2, 1, 2]               # tap 5 = (ky 1, kx 2), not flipped
    assert np.all(wf[:, 3:] == 0) and np.all(wf[:, :, 2:] == 0) and np.all(wb[:, 2:] == 0) and np.all(wb[:, :, 3:] == 0)
    assert (wf != 0).sum() == w.size == (wb != 0).sum()


@pytest.mark.parametrize("cid", [c.id for c in R.CASES if c.entry == "pool"])
def test_maxpool_matches_torch(cid):
    c = R.BY_ID[cid]
    inp = R.pool_inputs(c)
    x = torch.from_numpy(inp["x"]).requires_grad_(True)
    H, W = inp["x"].shape[-2:]
    to, ti = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    ref = R.plane_reference(c, inp)
    assert R.bits_differ(ref["y"], to.detach().numpy()) == 0
    ti = ti.numpy()
    OH, OW = ti.shape[-2:]
    ky = ti // W - (2 * np.arange(OH)[:, None] - 1)
    kx = ti % W - (2 * np.arange(OW)[None, :] - 1)
    assert np.array_equal(ref["idx"], (ky * 3 + kx).astype(np.uint8))
    if not c.special:                           # (torch's backward of a NaN window is the same routing; its inf * 0 is not)
        to.backward(torch.from_numpy(inp["dy"]))
        assert R.bits_differ(ref["dx"], x.grad.numpy()) == 0
    else:
        y, idx = ref["y"][0, 0, 1::2, 1], ref["idx"][0, 0, 1::2, 1]
        wins = R._special_windows()
        assert len(y) == len(wins) == R.N_SPECIAL
        n_nan = sum(bool(np.isnan(w).any()) for w in wins)
        assert np.isnan(y).sum() == n_nan == 7 and (y == -np.inf).sum() == 1
        for w, v, i in zip(wins, y, idx):
            if np.isnan(w).any():
                assert np.isnan(v) and i == np.flatnonzero(np.isnan(w))[-1]            # of several NaNs the last
            else:
                assert v == w.max() and i == int(np.argmax(w))                          # the first maximum
        assert set(idx.tolist()) >= {0, 4, 8}


def test_sampling_and_phases_match_slicing():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 3, 7, 9)).astype(F32)
    assert np.array_equal(R.subsample2(x), x[:, :, ::2, ::2])
    dy = rng.standard_normal((2, 3, 4, 5)).astype(F32)
    dx = R.subsample2_adjoint(dy, 7, 9)
    assert np.array_equal(dx[:, :, ::2, ::2], dy) and (dx != 0).sum() == (dy != 0).sum()
    assert np.vdot(R.subsample2(x).astype(np.float64), dy.astype(np.float64)) == np.vdot(x.astype(np.float64), dx.astype(np.float64))
    x = rng.standard_normal((2, 3, 4, 8)).astype(F32)
    xs = R.space_to_depth2(x)
    want = torch.stack([torch.from_numpy(x)[:, :, py::2, px::2] for py in (0, 1) for px in (0, 1)], dim=1).numpy()
    assert np.array_equal(xs, want) and np.array_equal(R.depth_to_space2(xs), x)
    assert not np.array_equal(R.space_to_depth2(x, "phase_swap"), xs)


# ---- the two kinds of input ----------------------------------------------------------------------------------------------------
def test_integer_inputs_are_exact_in_float32():
    """|x|, |w|, |dy| <= 3: every product is at most 9 and every partial sum at most 9 K < 2^24 in magnitude."""
    for c in R.CONV:
        inp = R.conv_inputs(c, "int")
        for k, v in inp.items():
            assert v.dtype == F32 and np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 3, (c.id, k)
        for op in ("fwd", "dx", "dw"):
            assert 9 * R.contraction(c, op) < 2 ** 24, (c.id, op)


REAL_SET = {
    "c3s1-nw1": ("fwd", "dx", "dw"), "c3s1-nw2x1": ("fwd", "dx", "dw"), "c3s2-nw2": ("fwd", "dx", "dw"), "c3s2-nw4": ("fwd", "dx", "dw"),
    "c1s1-nw4x2": ("fwd", "dx", "dw"), "c1s2-odd-zero": ("fwd", "dx", "dw"), "c3s1-w1": ("fwd", "dx", "dw"), "c3s2-h1": ("fwd", "dx", "dw"),
    "c7s1-h1w1": ("fwd", "dx", "dw"), "c3s2-rem": ("fwd", "dx", "dw"), "c3s1-p0": ("fwd", "dx", "dw"), "c3s2-p0": ("fwd", "dx", "dw"),
    "c1s1-p1": ("fwd", "dx", "dw"), "c1s2-p1": ("fwd", "dx", "dw"), "c3s1-p4": ("fwd", "dx", "dw"), "c3s2-p4": ("fwd", "dx", "dw"),
    "c5s2": ("fwd", "dx"), "c5s1-p0": ("fwd", "dx"), "c7s1": ("fwd", "dx", "dw"), "c7s2-general": ("fwd", "dx", "dw"),
    "wrw-uneven-tiles": (), "wrw-blocks-1024": ("fwd", "dx", "dw"), "wrw-reduce16-chains": (), "wrw-reduce64-chains": (), "wrw-s2-tiles": ("dw",),
    "wrw-1x1s2-tiles": ("dw",), "stem-c1-o8": ("fwd", "dx", "dw"), "stem-c2-o64": ("dw",), "stem-c3-o80": ("dw",),
    "stem-c3-o80-ow21": ("dw",), "stem-c4-o80": ("dw",), "stem-c3-o80-dyoff": ("dw",)}


def test_real_valued_set():
    """Which (case, op) pairs run real-valued: those whose largest bar stays under 0.125; every kernel family has at least one."""
    assert {c.id: R.real_ops(c) for c in R.CONV} == REAL_SET
    fams = set()
    for c in R.CONV:
        inp = R.conv_inputs(c, "real")
        assert all(0.5 <= abs(v) <= 1.0 for a in inp.values() for v in (a.min(), a.max(), np.abs(a).min()))
        for op in ("fwd", "dx", "dw"):
            if op not in c.ops or (op == "dw" and c.ks == 5):
                continue
            val, K, mag = R.conv_reference(c, inp, op)
            assert K.max() <= R.contraction(c, op), (c.id, op)
            assert (op in R.real_ops(c)) == (R.conv_bar(c, op, K, mag).max() < R.REAL_BAR_MAX), (c.id, op)
            if op in R.real_ops(c):
                fams |= {"convs_fwd_kernel<%d>" % R.nw_of(R.round_up(c.Cout, 16))} if op == "fwd" else \
                    {"convs_bwd_data_kernel<%d>" % R.nw_of(R.round_up(c.Cin, 16))} if op == "dx" else \
                    set(c.plan["kernels"]) | {"reduce<%d>" % c.plan["reduce"]}
    want = {k for c in R.CONV for k in c.kernels if k != "convs_pack_kernel"} | {"reduce<0>", "reduce<16>", "reduce<64>"}
    assert fams == want, sorted(want - fams)


# ---- the comparisons of the GPU test: correct results pass, mutants do not ----------------------------------------------------
@pytest.mark.parametrize("cid", CONV_IDS)
def test_unmutated_reference_passes_its_own_comparison(cid):
    c = R.BY_ID[cid]
    for kind in ("int", "real"):
        inp = R.conv_inputs(c, kind)
        for op in (c.ops if kind == "int" else R.real_ops(c)):
            if op == "dw" and c.ks == 5:
                continue
            ref = R.conv_reference(c, inp, op)
            ratio, bad = R.check_conv(c, op, kind, ref[0].astype(F32), inp, ref)
            assert not bad, bad


# (mutant, case, op, kinds it must be rejected in)
BOTH = ("int", "real")
MUTANTS = [
    ("drop_left", "c3s1-nw1", "fwd", BOTH), ("drop_right", "c3s1-nw1", "fwd", BOTH), ("drop_top", "c3s2-nw2", "fwd", BOTH),
    ("drop_bottom", "c3s2-nw2", "fwd", BOTH), ("drop_left", "c3s2-nw2", "dx", BOTH), ("drop_right", "c7s1", "dx", BOTH),
    ("drop_top", "c7s2-general", "dw", BOTH), ("drop_bottom", "stem-c1-o8", "dw", BOTH), ("drop_left", "stem-c3-o80", "dw", BOTH),
    ("drop_right", "c3s2-p0", "dw", BOTH),
    ("flip_taps", "c3s2-nw2", "dx", BOTH), ("flip_taps", "c7s1", "dx", BOTH),
    ("swap_parity", "c3s2-nw2", "dx", BOTH), ("swap_parity", "c1s2-odd-zero", "dx", BOTH),
    ("neg_div", "c3s2-p0", "dx", BOTH), ("neg_div", "c7s2-general", "dx", BOTH), ("neg_div", "c3s1-nw1", "dx", BOTH),
    ("zero_last_block", "c3s2-nw2", "fwd", BOTH), ("zero_last_block", "c3s1-nw2x1", "dx", BOTH), ("zero_last_block", "c7s1", "dw", BOTH),
    ("stem_ncob", "stem-c3-o80-dyoff", "dw", BOTH), ("stem_ncob", "stem-c3-o80-ow21", "dw", BOTH),
    ("drop_split", "c3s2-nw2", "dw", BOTH), ("drop_split", "stem-c3-o80", "dw", BOTH), ("drop_split", "wrw-uneven-tiles", "dw", ("int",)),
    ("drop_split", "wrw-reduce16-chains", "dw", ("int",)), ("drop_split", "wrw-reduce64-chains", "dw", ("int",)),
    ("drop_wave", "c3s1-nw1", "dw", BOTH), ("drop_wave", "c7s2-general", "dw", BOTH),
    ("leak_cols", "stem-c1-o8", "dw", BOTH), ("leak_cols", "stem-c2-o64", "dw", BOTH), ("leak_cols", "stem-c3-o80", "dw", BOTH),
    ("perm_group", "stem-c1-o8", "dw", BOTH), ("perm_group", "stem-c3-o80", "dw", BOTH),
    ("fp16", "c3s1-nw1", "fwd", ("real",)), ("fp16", "c3s2-nw2", "dx", ("real",)), ("fp16", "stem-c1-o8", "dw", ("real",)),
    ("fp16", "c1s2-odd-zero", "dw", ("real",))]


@pytest.mark.parametrize("mut,cid,op,kinds", MUTANTS)
def test_comparison_rejects_conv_mutant(mut, cid, op, kinds):
    c = R.BY_ID[cid]
    assert op in c.ops
    for kind in kinds:
        assert kind == "int" or op in R.real_ops(c), "a real-run mutant needs a case of the real-valued set"
        inp = R.conv_inputs(c, kind)
        got = R.conv_reference(c, inp, op, mut)[0].astype(F32)
        ratio, bad = R.check_conv(c, op, kind, got, inp)
        assert bad, (mut, cid, op, kind, ratio)


def test_fp16_is_invisible_to_the_integer_run():
    """Why there is a real-valued run: small integers pass through fp16 unchanged."""
    c = R.BY_ID["c3s1-nw1"]
    inp = R.conv_inputs(c, "int")
    assert not R.check_conv(c, "fwd", "int", R.conv_reference(c, inp, "fwd", "fp16")[0].astype(F32), inp)[1]


PLANE_MUTANTS = [("pool_last", "pool-special"), ("pool_last", "pool-6x8"), ("pool_nonan", "pool-special"), ("sub_odd_rows", "sub-vec"),
                 ("sub_odd_rows", "sub-odd"), ("phase_swap", "s2d-min"), ("phase_swap", "s2d-3x5")]


def _plane_inputs(c):
    return R.pool_inputs(c) if c.entry == "pool" else R.plane_inputs(c)


@pytest.mark.parametrize("mut,cid", PLANE_MUTANTS)
def test_comparison_rejects_plane_mutant(mut, cid):
    c = R.BY_ID[cid]
    inp = _plane_inputs(c)
    ref, got = R.plane_reference(c, inp), R.plane_reference(c, inp, mut)
    if mut == "phase_swap":                     # swapped both ways the round trip is still the identity: the phase tensor shows it
        assert R.bits_differ(got["xs"], ref["xs"]) and not R.bits_differ(got["back"], ref["back"])
    assert any(R.bits_differ(got[k], ref[k]) or R.unwritten(got[k]) for k in ref), (mut, cid)
    assert not any(R.bits_differ(ref[k], ref[k]) or R.unwritten(ref[k]) for k in ref)


def test_every_listed_mutant_is_tried():
    assert {m[0] for m in MUTANTS} | {m[0] for m in PLANE_MUTANTS} == {
        "drop_left", "drop_right", "drop_top", "drop_bottom", "flip_taps", "swap_parity", "neg_div", "zero_last_block", "stem_ncob",
        "drop_split", "drop_wave", "leak_cols", "perm_group", "fp16", "pool_last", "pool_nonan", "sub_odd_rows", "phase_swap"}


# ---- the table ----------------------------------------------------------------------------------------------------------------
def test_case_table_is_consistent():
    assert len(R.BY_ID) == len(R.CASES)
    for c in R.CONV:
        assert R.check_sconv(*c.geom) == 0, c.id
    fwd = [c for c in R.CONV if "fwd" in c.ops]
    assert {R.nw_of(R.round_up(c.Cout, 16)) for c in fwd} == {1, 2, 4} == {R.nw_of(R.round_up(c.Cin, 16)) for c in fwd}
    for attr in ("Cout", "Cin"):                # a padded channel count that is no multiple of 16 NW, with NW = 2 and NW = 4
        assert {R.nw_of(R.round_up(getattr(c, attr), 16)) for c in fwd if R.round_up(getattr(c, attr), 16) % (16 * R.nw_of(R.round_up(getattr(c, attr), 16)))} == {2, 4}
    assert any(c.Cin % 4 for c in fwd) and any(c.OW < 16 for c in fwd) and any(c.OW % 16 == 1 and c.OW > 16 for c in fwd)
    assert any(c.W == 1 for c in fwd) and any(c.H == 1 for c in fwd) and {c.B for c in fwd} >= {1, 3}
    assert any(c.s == 2 and c.W % 2 == 1 and c.W > 32 for c in fwd)                       # the odd parity class one column short
    assert any(c.ks == 1 and c.s == 2 for c in fwd) and any((c.H + 2 * c.p - c.ks) % c.s for c in fwd)
    assert {(c.ks, c.s, c.p) for c in fwd} >= {(3, 1, 0), (3, 2, 0), (1, 1, 1), (3, 1, 4), (3, 2, 4), (5, 2, 2)}
    dw = [c for c in R.CONV if "dw" in c.ops and c.ks != 5]
    gen = [c for c in dw if not c.plan["stem"]]
    assert {c.plan["kernels"][0] for c in gen} == {f"convs_wrw_kernel<{a}, {b}, {s}>" for a, b in ((1, 1), (3, 3), (1, 7)) for s in (1, 2)}
    assert any(c.Cout % 16 and c.Cin % 16 and c.OH % 4 and c.OW % 32 for c in gen)
    assert any(1 < c.plan["nsplit"] < c.plan["tiles"] and c.plan["tiles"] % c.plan["nsplit"] for c in gen)          # uneven tiles per split
    assert any(c.plan["nsplit"] == 1 and c.plan["ncob"] * c.plan["ncib"] >= 1024 and c.plan["tiles"] > 0 for c in gen)
    assert any(c.plan["tiles"] == 1 for c in gen)
    assert any(c.plan["reduce"] == 16 and c.plan["nsplit"] >= 64 and c.plan["nsplit"] % 64 for c in gen)
    assert any(c.plan["reduce"] == 64 and c.plan["nsplit"] >= 16 and c.plan["nsplit"] % 16 for c in gen)
    stem = [c for c in dw if c.plan["stem"]]
    assert {c.Cin for c in stem} == {1, 2, 3} and {c.Cout for c in stem} >= {8, 64, 80}
    assert any(c.OW < 32 for c in stem) and any(c.OW > 32 for c in stem) and all(c.OW % 4 == 0 for c in stem)
    near = [c for c in gen if c.ks == 7 and c.s == 2 and c.p == 3 and c.Cout == 80]
    assert {(c.Cin, c.OW % 4 == 0, c.offdy) for c in near} == {(3, False, 0), (4, True, 0), (3, True, 1)}
    off = R.BY_ID["stem-c3-o80-dyoff"]
    al = R.plan_wrw(*off.geom, dy_aligned=True)
    assert al["stem"] and not off.plan["stem"] and off.plan["ncob"] == 5 and al["ncob"] == 2
    assert off.plan["ws_bytes"] > al["ws_bytes"] and off.plan["query"] == off.plan["ws_bytes"] == al["query"]      # what the old plan overran
    shapes = {c.shape[2:] for c in R.CASES if c.entry == "pool"}
    assert any(h % 2 and w % 2 for h, w in shapes) and any(h % 2 == 0 and w % 2 == 0 for h, w in shapes)
    assert any(h == 1 for h, w in shapes) and any(w == 1 for h, w in shapes) and any(c.special for c in R.CASES if c.entry == "pool")
    sub = [c for c in R.CASES if c.entry == "sub"]
    assert {(R.sub_vec(c.shape[3], c.offx, c.offy), c.shape[3] % 8 == 0) for c in sub} == {(True, True), (False, True), (False, False)}
    assert any(c.shape[2] % 2 and c.shape[3] % 2 for c in sub)
    assert {c.shape for c in R.CASES if c.entry == "s2d"} >= {(1, 1, 2, 8)} and any(c.shape[0] > 1 and c.shape[1] > 1 for c in R.CASES if c.entry == "s2d")
    assert any(2 * c.ks ** 2 * c.Cin * c.Cout > 1024 * 256 for c in fwd)                 # the pack kernel's grid cap: a second trip of its loop
    # every conv view but dy sits 0..3 floats off, and over the table every offset occurs
    assert {c.off(k) for c in R.CONV for k in ("x", "w", "y", "dx", "dw", "wf", "wb", "ws")} == {0, 1, 2, 3}


def test_restated_plan_matches_the_workspace_query():
    """uaps_convs_wrw_workspace_bytes is host-only: for every weight-gradient case it reports the restated plan's `query` -- the form's
    own need, or for a stem shape the larger of the two forms' (it cannot see dy)."""
    from uaps_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libuaps_hip.so is not built")
    L = _lib.lib()
    n, seen_larger = C.c_size_t(), 0
    for c in R.CONV:
        if "dw" not in c.ops or c.ks == 5:
            continue
        assert L.uaps_convs_wrw_workspace_bytes(*c.geom, C.byref(n)) == 0
        assert n.value == c.plan["query"] >= c.plan["ws_bytes"], c.id
        seen_larger += c.plan["query"] > c.plan["ws_bytes"]
    assert seen_larger >= 1                     # a stem-form case whose general plan needs more than it does
    # the workload's stem (BASELINE.json configs[4]): the stem form needs the most there, the general plan 36 splits of 49 x 64 x 16
    g = R.plan_wrw(16, 3, 64, 640, 640, 7, 2, 3, dy_aligned=False)
    assert L.uaps_convs_wrw_workspace_bytes(16, 3, 64, 640, 640, 7, 2, 3, C.byref(n)) == 0
    assert n.value == 1024 * 64 * 160 * 4 == g["query"] and g["ws_bytes"] == 36 * 49 * 64 * 16 * 4 and g["nsplit"] == 36
    assert L.uaps_convs_wrw_workspace_bytes(2, 6, 20, 9, 19, 5, 2, 2, C.byref(n)) == 0                      # the query does not know the 5x5 refusal


def _built():
    from uaps_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libuaps_hip.so is not built")
    return norm_act_kernel_symbols(_lib.LIB_PATH, kernel_pattern(R.KERNEL_NAMES))


def test_cases_cover_every_kernel_and_name_none_that_does_not_exist():
    built = _built()
    assert len(built) == 21, sorted(built)
    named = set().union(*(c.kernels for c in R.CASES))
    assert named == built, ("no case reaches", sorted(built - named), "no such kernel", sorted(named - built))


def test_every_kernel_of_the_source_is_in_the_filter():
    GLOBAL = r"__global__(?:\s+__launch_bounds__\([^)]*\))?\s+void\s+(\w+)\s*\("
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uaps_amd", "csrc", "conv_strided.hip")
    assert set(re.findall(GLOBAL, open(src).read())) == set(R.KERNEL_NAMES)


def test_removing_a_case_uncovers_its_kernel():
    built = _built()
    sole = {}
    for k in built:
        owners = [c.id for c in R.CASES if k in c.kernels]
        assert owners, k
        if len(owners) == 1:
            sole[k] = owners[0]
    for k, cid in sole.items():
        named = set().union(*(c.kernels for c in R.CASES if c.id != cid))
        assert k in built - named
