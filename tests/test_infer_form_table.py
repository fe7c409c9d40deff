"""The inference-side table of tests/infer_form_cases.py on the CPU: from the table, the restated launch rules and the references alone,
every kernel of csrc/tta.hip, tiled.hip and curves.hip in the built code object is named by a case (and nothing else is), every form
tests/test_gpu_infer_forms.py is there to reach is reached, the references agree with the independent ones the suite already has, every
derived bar is at or below the existing sweeps' and every mask comparison within the cap, and the GPU test's comparison rejects every
mutant of the walks."""
import os

import numpy as np
import pytest
import torch

import curves_ref as CR
import infer_form_cases as E
import tiled_ref as TR
import tta_ref as TT
from test_bn_ref import kernel_pattern, norm_act_kernel_symbols


def _cases(form):
    got = [c for c in E.CASES if form in c.forms]
    assert got, form
    return got


def test_ids_are_unique_every_case_names_its_form_and_the_rules_are_restated():
    ids = [c.id for c in E.CASES]
    assert len(ids) == len(set(ids)) and all(c.forms for c in E.CASES)
    assert (E.span(1), E.span(4)) == (1024, 4096)
    assert E.units_per_group(3, 1367, True) == 3 and E.units_per_group(3, 4096, True) == 1 and E.units_per_group(3, 4096, False) == 4
    assert E.units_per_group(2, 64, True) == 4 and E.groups(3, 1367, True) == 2 and E.groups(3, 4096, True) == 6
    assert [E.rounds_run(n, 1) for n in (512, 513, 1024, 1025)] == [1, 2, 2, 1] and [E.wpi(n, 1) for n in (512, 513, 1024, 1025)] == [1, 1, 1, 2]
    assert [E.rounds_run(n, 4) for n in (2048, 2052, 4096, 4100)] == [1, 2, 2, 1] and [E.wpi(n, 4) for n in (2048, 2052, 4096, 4100)] == [1, 1, 1, 2]
    assert E.al16(1, 8) is False and E.al16(2, 8) and E.al16(4, 4) and not E.al16(3, 1) and E.al16(16, 1)


def test_census_every_kernel_of_the_three_files_is_named_and_nothing_else():
    from uaps_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libuaps_hip.so is not built")
    built = norm_act_kernel_symbols(_lib.LIB_PATH, kernel_pattern(E.KERNEL_NAMES))
    named = set().union(*(c.kernels for c in E.CASES))
    assert not built - named - set(E.UNREACHABLE), f"built, reached by no case: {sorted(built - named)}"
    assert not named - built, f"named by a case, not in the code object: {sorted(named - built)}"
    assert not set(E.UNREACHABLE) & named and not E.UNREACHABLE                      # (none is expected)
    assert len(built) == 15 + 17 + 38


# ---- test-time augmentation ----------------------------------------------------------------------------------------------------------
def test_tta_forms_are_reached():
    for C in range(2, 9):
        assert {c.V for c in _cases(f"tta-C{C}-V4") + _cases(f"tta-C{C}-V1")} == {4, 1}
        assert all(c.arg("C") == C and c.arg("B", 2) == 2 for c in _cases(f"tta-C{C}-V4"))
    for way, why in (("W", lambda c: c.arg("W") % 4 != 0 and not c.offs), ("probs", lambda c: c.offs == (("probs", 1),)),
                     ("mask", lambda c: c.offs == (("mask", 1),)), ("conf", lambda c: c.offs == (("conf", 1),))):
        (c,) = _cases(f"tta-V1-by-{way}")
        assert c.V == 1 and why(c) and c.arg("C") == 4
    assert {c.outs for c in _cases("tta-V4-null-outputs")} == {("mask",), ("conf",), ("probs",)} and all(c.V == 4 for c in _cases("tta-V4-null-outputs"))
    assert len(_cases("tta-S1")[0].arg("sizes")) == 1 and len(_cases("tta-S8")[0].arg("sizes")) == 8
    (c,) = _cases("tta-identity")
    assert {(1, 6), (4, 1), (8, 12)} <= set(c.arg("sizes")) and (c.arg("H"), c.arg("W")) == (8, 12)
    i0, i1, l0, l1 = E.corners(8, 8)                                                 # r = 1: the pixel itself, l1 = 0
    assert i0.tolist() == list(range(8)) and not l1.any() and (l0 == 1).all()
    i0, i1, l0, l1 = E.corners(1, 8)                                                 # one source row
    assert not i0.any() and not i1.any() and not l1.any()
    i0, i1, l0, l1 = E.corners(12, 1)                                                # one output row: the ratio is 0
    assert i0.tolist() == [0] and l1.tolist() == [0]
    assert _cases("tta-H1")[0].arg("H") == 1 and _cases("tta-W1")[0].arg("W") == 1 and _cases("tta-W1")[0].V == 1
    H, W = 8, 12
    assert all(h < H and w < W for h, w in _cases("tta-upscale-only")[0].arg("sizes"))
    assert all(h > H and w > W for h, w in _cases("tta-downscale-only")[0].arg("sizes"))
    assert _cases("tta-flip0")[0].arg("flip") == 0 and _cases("tta-B1")[0].arg("B") == 1
    (c,) = _cases("tta-ties")
    for z in E.inputs(c).values():
        assert np.array_equal(z[:, 1], z[:, 3]) and (z[:, 1:2] > np.delete(z, (1, 3), axis=1)).all()
    v = E.reference(c)["probs"][0]
    assert np.array_equal(v[:, 1], v[:, 3]) and (v.argmax(axis=1) == 1).all()
    assert _cases("tta-saturated")[0].arg("gain") == 60.0
    # the interior fractions are real fractions: l1 takes many values
    assert len(np.unique(E.corners(6, 12)[3])) > 6


def test_tta_views_forms_are_reached():
    assert {c.arg("Cin") for c in E.CASES if c.entry == "tta_views"} == {1, 3}
    down, up, ident = _cases("views-down")[0], _cases("views-up")[0], _cases("views-identity")[0]
    assert down.arg("h") < down.arg("H") and up.arg("h") > up.arg("H") and (ident.arg("h"), ident.arg("w")) == (ident.arg("H"), ident.arg("W"))
    assert _cases("views-h1")[0].arg("h") == 1 and _cases("views-w1")[0].arg("w") == 1
    (c,) = _cases("views-flip0")
    assert c.arg("flip") == 0 and c.arg("buf2") == 1
    assert any(c.off("x") % 2 and c.off("out") % 2 for c in E.CASES if c.entry == "tta_views")
    v, b = E.reference(ident)["out"]
    assert np.array_equal(v, E.inputs(ident)["x"].astype(np.float64))                # the identity is exact


# ---- tiled inference -----------------------------------------------------------------------------------------------------------------
def test_tile_cut_forms_are_reached():
    for form, ax in (("cut-H1", "H"), ("cut-W1", "W")):
        assert _cases(form)[0].arg(ax) == 1
    for c in _cases("cut-mirror-periods"):
        n, t = (c.arg("H"), c.arg("tile")[0]) if c.arg("H") < 16 else (c.arg("W"), c.arg("tile")[1])
        assert n == 5 and t > 2 * (n - 1) + 1                                         # the mirror wraps more than one period
        assert [E.mirror(i, 5) for i in range(16)] == [0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    (c,) = _cases("cut-tile-is-image")
    assert (c.arg("H"), c.arg("W")) == c.arg("tile") and E.n_tiles(c) == 2
    (c,) = _cases("cut-clamped-last")
    (ys, _), (xs, _) = E.tile_geometry(c)
    assert ys == [0, 12, 24, 25] and xs == [0, 12, 24, 34]
    (c,) = _cases("cut-window")
    T = E.n_tiles(c) // 2
    assert 0 < c.arg("g0") < T < c.arg("g1") < 2 * T
    assert {c.arg("Cin") for c in E.CASES if c.entry == "tile_cut"} == {1, 3}
    assert all(c.off("x") % 2 or c.off("out") % 2 for c in E.CASES if c.entry == "tile_cut")


def _boundaries(c):
    """The chunk boundaries of a fold case as (tile, position in the tile row, tiles a row, tiles an image)."""
    (ys, _), (xs, _) = E.tile_geometry(c)
    T, nx, G, tpc = len(ys) * len(xs), len(xs), E.n_tiles(c), c.arg("tpc")
    return [(g, g % T % nx, nx, T) for g in range(tpc, G, tpc)], G, T, tpc


def test_tile_fold_forms_are_reached():
    for n in (1, 2):
        assert {c.V for c in _cases(f"fold-C0-maps{n}-V4") + _cases(f"fold-C0-maps{n}-V1")} == {4, 1}
        assert all(c.arg("C") == 0 and c.arg("n_maps") == n for c in _cases(f"fold-C0-maps{n}-V1"))
    for C in range(2, 9):
        assert {c.V for c in _cases(f"fold-C{C}-V4") + _cases(f"fold-C{C}-V1")} == {4, 1}
    assert _cases("fold-C4-maps2")[0].arg("n_maps") == 2 and _cases("fold-C4-maps2")[0].V == 4
    for way in ("W", "probs", "mask", "conf", "map"):
        (c,) = _cases(f"fold-V1-by-{way}")
        assert c.V == 1 and len(c.offs) == (0 if way == "W" else 1) and (way != "W" or c.arg("W") % 4)
    (c,) = _cases("fold-overlap0")
    assert c.arg("overlap") == (0, 0) and set(np.unique(E.tile_geometry(c)[0][1].sum(0))) == {1}
    (c,) = _cases("fold-half-overlap-odd")
    assert c.arg("tile") == (7, 7) and c.arg("overlap") == (3, 3)
    (c,) = _cases("fold-nine-tiles")
    (ys, cy), (xs, cx) = E.tile_geometry(c)
    assert set(np.unique(cy.sum(0))) == {1, 2, 3} and set(np.unique(cx.sum(0))) == {1, 2, 3}
    for orig, cov in ((ys, cy), (xs, cx)):                                             # regular tiles k - 1 and k, and the clamped last one
        p = int(np.nonzero(cov.sum(0) == 3)[0][0])
        assert cov[:, p].tolist() == [False, True, True, True] and orig[-1] not in [i * (orig[1] - orig[0]) for i in range(4)]
    assert (np.outer(cy.sum(0), cx.sum(0)) == 9).any()
    (c,) = _cases("fold-th-ne-tw")
    assert c.arg("tile")[0] != c.arg("tile")[1]
    (c,) = _cases("fold-one-chunk")
    assert c.arg("tpc") == E.n_tiles(c)
    (c,) = _cases("fold-32-chunks")
    assert E.n_tiles(c) == 32 and c.arg("tpc") == 1
    c = E.BY_ID["fold-c4-v4"]                                                           # the common geometry
    bounds, G, T, tpc = _boundaries(c)
    assert G % tpc and any(pos != 0 for _, pos, _, _ in bounds)                         # a short last chunk; a boundary inside a tile row
    assert any((g - tpc) < T < g for g, *_ in bounds)                                  # a chunk holds tiles of both images
    (c,) = _cases("fold-image-below-tile")
    assert c.arg("H") < c.arg("tile")[0] and c.arg("W") < c.arg("tile")[1]
    folds = [c for c in E.CASES if c.entry == "tile_fold"]
    assert {c.arg("window", "asym") for c in folds} == {"asym", "uniform", "triangle", "gauss"}
    for c in folds:
        inp = E.inputs(c)
        if c.arg("window", "asym") == "asym":
            assert not np.array_equal(inp["wy"], inp["wy"][::-1]) and not np.array_equal(inp["wx"], inp["wx"][::-1])
            assert inp["wy"].min() >= 0.1 and inp["wx"].max() <= 1.0 and not np.array_equal(inp["wy"][:7], inp["wx"][:7])


# ---- curves --------------------------------------------------------------------------------------------------------------------------
def _first_wave_keys(c):
    """The distinct bins among key[0] of the 64 lanes of the first wave, class row 0."""
    S = E.inputs(c)["scores"]
    V = c.V
    px = np.arange(64) * V
    return len(set(CR.bins_of(S[0, c.arg("classes")[0]].reshape(-1)[px], c.arg("bins", 64), c.arg("lo", 0.0), c.arg("hi", 1.0)).tolist()))


def test_score_forms_are_reached():
    for C in range(1, 9):
        for q in (0, 1):
            (a,), (b,) = _cases(f"score-C{C}-V4-q{q}"), _cases(f"score-C{C}-V1-q{q}")
            assert (a.V, b.V, a.arg("C"), b.arg("qsum")) == (4, 1, C, q)
    for d in (E.U8, E.I32, E.I64):
        assert {c.arg("C") for c in _cases(f"score-dtype{d}-V4")} == {1, 3, 8} == {c.arg("C") for c in _cases(f"score-dtype{d}-V1")}
        assert all(c.V == 4 for c in _cases(f"score-dtype{d}-V4")) and all(c.V == 1 and c.offs == (("target", c.off("target")),) for c in _cases(f"score-dtype{d}-V1"))
    assert _cases("score-V1-by-HW")[0].arg("H") * _cases("score-V1-by-HW")[0].arg("W") % 4 and not _cases("score-V1-by-HW")[0].offs
    assert _cases("score-V1-by-scores")[0].offs == (("scores", 3),) and _cases("score-V1-by-region-labels")[0].offs == (("rl", 1),)
    tg = {c.arg("tdt"): c for c in _cases("score-V1-by-target")}
    assert tg[E.U8].off("target") % 2 == 1 and tg[E.I64].off("target") * 8 % 16 == 8
    assert all(c.V == 1 for c in _cases("score-V1-by-target") + _cases("score-V1-by-scores") + _cases("score-V1-by-region-labels"))
    assert sorted((c.arg("H") * c.arg("W"), c.arg("B")) for c in _cases("score-span-V1")) == [(512, 2), (513, 3), (1024, 2), (1025, 3)]
    assert sorted((c.arg("H") * c.arg("W"), c.arg("B")) for c in _cases("score-span-V4")) == [(2048, 2), (2052, 3), (4096, 2), (4100, 3)]
    assert all(c.V == 1 for c in _cases("score-span-V1")) and all(c.V == 4 for c in _cases("score-span-V4"))
    for c in _cases("score-span-V1") + _cases("score-span-V4"):       # the last pixel of every image: counted in the class row, a NaN in the top row
        inp, ref, bins = E.inputs(c), E.reference(c), c.arg("bins", 64)
        S, t = inp["scores"].reshape(c.arg("B"), 2, -1), inp["target"].reshape(c.arg("B"), -1)
        assert np.isnan(S[:, 0, -1]).all() and (S[:, 1, -1] == 0.25).all() and ((t[:, -1] == 0) | (t[:, -1] == 1)).all()
        assert c.arg("classes") == (1,) and c.arg("top", 1) == 1 and (ref["nan"][:, 1] > 0).all()
        assert ref["hist"][:, 0, :, bins // 4].sum(axis=1).min() > 0 and ref["hist"].sum(axis=(1, 2, 3)).min() > 0
    for k in (1, 4, 5, 64):
        assert {c.V for c in _cases(f"score-keys{k}")} == {4, 1} and all(_first_wave_keys(c) == k for c in _cases(f"score-keys{k}"))
    assert E.PEEL == 4
    for form, k in (("score-qsum-single-lane", 64), ("score-qsum-several-lanes", 1)):
        for c in _cases(form):
            assert _first_wave_keys(c) == k and c.arg("qsum") == 1 and c.arg("lo") < 0
            assert (E.inputs(c)["scores"] < 0).any() and (E.reference(c)["qsum"] < 0).any()
    assert {E.units_per_group(c.R, c.arg("bins"), True) for c in _cases("score-odd-upg")} == {3, 1}
    for c in _cases("score-odd-upg"):
        upg = E.units_per_group(c.R, c.arg("bins"), True)
        assert c.R >= 2 and any((2 * r) // upg != (2 * r + 1) // upg for r in range(c.R)) and (E.reference(c)["nan"] > 0).all()
    assert {c.arg("C") for c in _cases("score-from-logits")} == {1, 2, 5} and all(c.arg("from_logits") == 1 for c in _cases("score-from-logits"))
    (c,) = _cases("score-logit-ties")
    S = E.inputs(c)["scores"]
    P = CR.probabilities(S, True)
    assert ((np.sort(P, axis=1)[:, -1] == np.sort(P, axis=1)[:, -2]).mean() > 0.5) and (np.sort(S, axis=1)[:, -1] > np.sort(S, axis=1)[:, -2]).all()
    assert _cases("score-top-alone")[0].arg("classes") == () and _cases("score-classes-alone")[0].arg("top") == 0
    assert _cases("score-unsorted-classes")[0].arg("classes") == (3, 1)
    for c in (c for c in E.CASES if c.entry == "score" and (c.pattern == "ignored" or c.arg("ignored"))):
        t = E.inputs(c)["target"].astype(np.int64)
        assert (t == 255).any() and (t == max(c.arg("C"), 2)).any() and (c.arg("tdt", E.I64) == E.U8 or (t == -1).any())
    assert all(len(_cases(f"score-bins{b}")) == 1 for b in (2, 15, 255, 256, 257, 1024, 4096))


def test_region_forms_are_reached():
    for C in (1, 4, 8):
        assert {c.V for c in _cases(f"regions-C{C}")} == {4, 1}
    for c in _cases("regions-counts"):
        inp = E.inputs(c)
        rl, cnt, tab = inp["rl"], inp["rcount"], inp["rtable"]
        Mg = tab.shape[1]
        assert cnt.tolist() == [Mg - 1, 0, -1, Mg + 3]
        assert (rl == 0).any() and (rl < 0).any() and (rl == Mg).any() and (rl > Mg).any() and cnt[0] < Mg
        classes = set(c.arg("classes"))
        rows = [(int(tab[0, r, 0]) in classes, int(tab[0, r, 1]) > 0) for r in range(cnt[0])]
        assert (False, True) in rows and (True, False) in rows and rows[0] == (True, True) and rows[-1][1]      # between the counted ones
        ref = E.reference(c)
        assert ref["n_regions"][0].sum() > 0 and not ref["n_regions"][1:3].any() and ref["n_regions"][3].sum() > 0 and ref["pro_sum"][0].any()
    (c,) = _cases("regions-many-groups")
    assert E.groups(c.R, c.arg("bins"), True) > 1
    pers = {}
    for b in (2, 255, 257, 1000, 4096):
        (c,) = _cases(f"pro-bins{b}")
        per = -(-b // 256)
        pers[b] = (per, -(-b // per), b % per)
        assert E.reference(c)["pro_sum"].any()
    assert pers == {2: (1, 2, 0), 255: (1, 255, 0), 257: (2, 129, 1), 1000: (4, 250, 0), 4096: (16, 256, 0)}      # (bins a lane, lanes used, ragged)


def test_plane_forms_are_reached():
    for V in (4, 1):
        cs = _cases(f"plane-dtypes-V{V}")
        assert {(c.arg("pdt"), c.arg("tdt")) for c in cs} == {(p, t) for p in (1, 4, 8) for t in (1, 4, 8)} and all(c.V == V for c in cs)
        assert _cases(f"plane-q0-V{V}") and _cases(f"plane-q1-V{V}")
    for c in (c for c in E.CASES if c.entry == "plane"):
        s = E.inputs(c)["scores"]
        assert (c.arg("lo"), c.arg("hi")) == (-2.5, 7.0) and (s < -2.5).any() and (s > 7).any() and np.isposinf(s).any() and np.isneginf(s).any()
        assert np.isnan(s).any() and E.reference(c)["nan"].sum() > 0
        assert len(E.fma_sensitive(c.arg("bins"), -2.5, 7.0)) > 0 and np.isin(E.fma_sensitive(c.arg("bins"), -2.5, 7.0)[:40], s).all()


# ---- the references agree with the independent ones ----------------------------------------------------------------------------------
def test_walks_agree_with_the_references_the_suite_already_has():
    for c in (c for c in E.CASES if c.entry == "tta_fold"):
        zs = [torch.from_numpy(np.array(z)) for z in E.inputs(c).values()]
        v = E.reference(c)["probs"][0]
        for other in (TT.fold, TT.fold_gather):                                        # float64 coordinates: apart by the fp32 source coordinate
            assert np.abs(other(zs, (c.arg("H"), c.arg("W")), bool(c.arg("flip", 1))).numpy() - v).max() <= TT.TAU_SUM, c.id
    for c in (c for c in E.CASES if c.entry == "tta_views"):
        x = torch.from_numpy(np.array(E.inputs(c)["x"]))
        assert np.abs(TT.views(x, (c.arg("h"), c.arg("w")), False).numpy() - E.reference(c)["out"][0]).max() <= TT.TAU_VIEWS, c.id
    for c in (c for c in E.CASES if c.entry == "tile_cut"):
        x = torch.from_numpy(np.array(E.inputs(c)["x"]))
        g0, g1 = c.arg("g0", 0), c.arg("g1", None) or E.n_tiles(c)
        assert np.array_equal(TR.cut(x, c.arg("tile"), c.arg("overlap")).numpy()[g0:g1], E.reference(c)["out"]), c.id
    for c in (c for c in E.CASES if c.entry == "tile_fold"):
        inp = E.inputs(c)
        z = torch.from_numpy(np.array(inp["z"])) if c.arg("C") else None
        maps = [torch.from_numpy(np.array(inp[f"m{m}"])) for m in range(c.arg("n_maps", 0))]
        probs, blended = TR.fold(z, (c.arg("B", 2), c.arg("H"), c.arg("W")), c.arg("tile"), c.arg("overlap"), inp["wy"], inp["wx"], maps) if z is not None \
            else _maps_only(c, inp, maps)
        ref = E.reference(c)
        if z is not None:
            assert np.abs(probs.numpy() - ref["probs"][0]).max() <= TR.TAU, c.id
        for m, t in enumerate(blended):
            assert np.abs(t.numpy() - ref[f"map{m}"][0]).max() <= TR.TAU, c.id
    for c in (c for c in E.CASES if c.entry in ("score", "plane")):                    # curves_ref against the second restatement, exactly
        ref, w = E.reference(c), E.walk(c)
        assert set(ref) == set(w) and all(ref[k].tobytes() == w[k].tobytes() and ref[k].dtype == w[k].dtype for k in ref), c.id
    e = CR.edge_values((15, 255, 257))
    for bins, lo, hi in ((15, 0.0, 1.0), (257, 0.0, 1.0), (255, -2.5, 7.0)):           # and curves_ref against its own scalar walk
        s = e[~np.isnan(e)]
        assert CR.bins_of(s, bins, lo, hi).tolist() == [CR.bin_scalar(v, bins, lo, hi) for v in s]


def _maps_only(c, inp, maps):
    """tiled_ref.fold needs class logits: blend the maps beside a dummy two-class tensor."""
    z = torch.zeros(maps[0].shape[0], 2, *c.arg("tile"))
    return TR.fold(z, (c.arg("B", 2), c.arg("H"), c.arg("W")), c.arg("tile"), c.arg("overlap"), inp["wy"], inp["wx"], maps)


def test_bars_are_at_or_below_the_existing_ones_and_masks_within_the_cap():
    assert E.MAX_EXCLUDED == TT.MAX_EXCLUDED == TR.MAX_EXCLUDED
    limit = dict(tta_fold=TT.TAU_SUM, tta_views=TT.TAU_VIEWS, tile_fold=TR.TAU)
    largest = {}
    for c in (c for c in E.CASES if c.entry in limit):
        for k, b in E.bars(c).items():
            assert np.isfinite(b).all() and float(b.max()) <= limit[c.entry], (c.id, k, float(b.max()), limit[c.entry])
            largest[c.entry, k] = max(largest.get((c.entry, k), 0.0), float(b.max()))
        if c.arg("C") and c.pattern != "ties":
            assert E.margin(c) <= min(TT.MARGIN, TR.MARGIN)                            # a narrower band than the existing sweeps exclude
            assert E.excluded(c) <= E.MAX_EXCLUDED, (c.id, E.excluded(c))
    print("largest bars:", {f"{e}.{k}": f"{v:.3e}" for (e, k), v in sorted(largest.items())})


# ---- the comparison accepts the walks and rejects every mutant -----------------------------------------------------------------------
def _got(c, mut=""):
    w = E.walk(c, mut)
    return E.as_got(c, w) if c.entry not in ("score", "plane") else w


def _own(c):
    return E.walk(c)["probs"][0].astype(np.float32) if c.entry in ("tta_fold", "tile_fold") and c.arg("C") else None


def test_the_comparison_accepts_every_reference():
    for c in E.CASES:
        bad, ratios = E.compare(c, _got(c), _own(c))
        assert not bad and all(v <= 1 for v in ratios.values()), (c.id, bad)
    c = E.BY_ID["tta-c4-v4"]                                                            # wrong types, shapes and sets of outputs
    g = _got(c)
    assert E.compare(c, {k: v for k, v in g.items() if k != "conf"})[0] and E.compare(c, dict(g, probs=g["probs"].astype(np.float64)))[0]
    assert E.compare(c, dict(g, mask=g["mask"].astype(np.int32)))[0] and E.compare(c, dict(g, probs=g["probs"][:1]))[0]
    hi = dict(g, mask=g["mask"].copy())
    hi["mask"][0, 0, 0] = (hi["mask"][0, 0, 0] + 1) % 4
    assert E.compare(c, hi)[0]
    nan = dict(g, probs=g["probs"].copy())
    nan["probs"][1, 2, 3, 4] = np.nan
    assert E.compare(c, nan)[0]
    c = E.BY_ID["tta-ties"]                                                             # the higher of two bit-identical classes
    g = _got(c)
    assert (g["mask"] == 1).all() and E.compare(c, dict(g, mask=np.full_like(g["mask"], 3)))[0]
    c = E.BY_ID["views-noflip"]                                                         # flip == 0 that writes the second half
    g = _got(c)
    g["out"] = np.concatenate([g["out"][:2], g["out"][:2]])
    assert E.compare(c, g)[0]
    c = E.BY_ID["score-regions-c4-v4"]                                                  # pro_sum is held bit for bit
    g = {k: v.copy() for k, v in _got(c).items()}
    i = tuple(np.argwhere(g["pro_sum"] > 0)[0])
    g["pro_sum"][i] = np.nextafter(g["pro_sum"][i], np.inf)
    assert E.compare(c, g)[0]


@pytest.mark.parametrize("mut", sorted(E.MUTANTS))
def test_every_mutant_is_rejected(mut):
    what, entries = E.MUTANTS[mut]
    caught = []
    for c in (c for c in E.CASES if c.entry in entries):
        if mut == "swap_windows" and c.arg("tile")[0] != c.arg("tile")[1]:
            continue
        if E.compare(c, _got(c, mut), _own(c))[0]:
            caught.append(c.id)
            if len(caught) == 3:
                break
    print(f"{mut} ({what}): rejected by {', '.join(caught)}")
    assert caught, f"no case rejects: {what}"
