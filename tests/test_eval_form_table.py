"""The evaluation-chain table of tests/eval_form_cases.py on the CPU: from the table, the restated dispatch facts and the references'
own outputs alone, every form of csrc/instances.hip, surface.hip and match.hip that tests/test_gpu_eval_forms.py is there to reach is
reached by a case, every census condition holds, and the GPU test's comparison rejects one subtle mistake per family planted in a copy
of the reference's output."""
import numpy as np
import pytest

import eval_form_cases as E
import instances_ref as I
import match_ref as M
import surface_ref as S


def _cases(form):
    return [c for c in E.CASES if form in c.forms]


def test_ids_are_unique_and_every_case_names_its_form():
    ids = [c.id for c in E.CASES]
    assert len(ids) == len(set(ids))
    assert all(c.forms for c in E.CASES)
    assert {f for c in E.CASES for f in c.forms} == set(E.FORMS) and len(set(E.FORMS)) == len(E.FORMS)      # every form has its case
    assert E.segments(16) == (1, 16) and E.segments(17) == (2, 9) and E.segments(33) == (3, 11) and E.segments(241) == (16, 16)
    assert E.segments(257) == (16, 17) and E.segments(1) == (1, 1) and E.segments(4096) == (16, 256)
    assert E.match_v(60, 0, 0) == 4 and E.match_v(60, 1, 0) == 1 and E.match_v(60, 0, 2) == 1 and E.match_v(63, 0, 0) == 1 and E.match_v(60, 4, 8) == 4
    assert (E.match_span(4), E.match_span(1)) == (1024, 256)
    assert [E.first_differing_pass(0, 1 << k) for k in (24, 16, 15, 8, 7, 0)] == [0, 0, 1, 1, 2, 2] and E.first_differing_pass(9, 9) is None


# ---- labelling -----------------------------------------------------------------------------------------------------------------------
def test_labelling_scan_runs_a_second_round_with_survivors_on_both_sides():
    cases = _cases("scan-multi-round")
    assert {c.arg("min_area") for c in cases} == {1, 3}
    for c in cases:
        B, H, W = c.shape
        assert E.chunks(H, W) == 1029 and E.scan_rounds(E.chunks(H, W)) == 2 and E.chunks(H, W) % 4 != 0
        ref = E.reference(c)
        for b in range(B):
            n = int(ref["count"][b])
            assert 0 < n <= c.arg("max_instances")                      # (the table is complete: its first pixels tell the chunks)
            ch = ref["table"][b, :n, 6] // E.CHUNK
            assert (ch < 1024).sum() > 0 and (ch == 1024).sum() > 0 and (ch > 1024).sum() > 0, (c.id, b)
            assert (ref["table"][b, :n, 1] >= c.arg("min_area")).all()
        assert all(c.off(k) % 2 == 1 for k in ("labels", "count", "mask", "table"))


def test_labelling_carries_meet_an_image_boundary():
    cases = _cases("carry-image-boundary")
    assert {c.shape for c in cases} == {(3, 9, 64), (3, 8, 72)} and {c.pattern for c in cases} == {"full", "rows2", "full_empty_full"}
    for c in cases:
        B, H, W = c.shape
        HW = H * W
        assert HW % 64 == 0 and HW % E.LABEL_SPAN != 0 and HW < E.LABEL_SPAN < B * HW      # whole groups; wave 0 holds images 0 and 1
        ref = E.reference(c)
        want = {"full": [1, 1, 1], "rows2": [H] * 3, "full_empty_full": [1, 0, 1]}[c.pattern]
        assert ref["count"].tolist() == want
        if c.pattern != "rows2":
            assert ref["table"][0, 0, 1] == HW and ref["table"][2, 0, 1] == HW and ref["table"][0, 0, 6] == ref["table"][2, 0, 6] == 0
            assert ref["table"][0, 0, 7] != ref["table"][2, 0, 7]                             # the maps' sums tell the images apart


def test_labelling_seams_wide_classes_overflow_and_maps():
    seams = _cases("seam-ragged")
    assert {(c.shape[1] % E.TILE, c.shape[2] % E.TILE) for c in seams} >= {(1, 15), (1, 0), (0, 1), (15, 2)}
    assert {c.pattern for c in seams} == {"spiral", "comb", "diagonal", "corners", "links"} and {c.arg("connectivity") for c in seams} == {4, 8}
    for c in (c for c in seams if c.pattern == "links"):                                     # one component per pair, diagonal ones under 8 only
        m, lab = E.inputs(c)["mask"][0], E.reference(c)["labels"][0]
        n_rows, n_cols = len(range(E.TILE, c.shape[1], E.TILE)), len(range(E.TILE, c.shape[2], E.TILE))
        assert (m > 0).sum() == 6 * (n_rows + n_cols) > 0
        assert lab.max() == (3 if c.arg("connectivity") == 8 else 5) * (n_rows + n_cols)
    assert all(E.reference(c)["count"].max() <= c.arg("max_instances") for c in seams)
    wide = _cases("int64-classes")
    assert {c.arg("background") for c in wide if c.entry == "label"} == {-5, 2 ** 32 + 1, 7, None}
    for c in (c for c in wide if c.entry == "label"):
        m, lab = E.inputs(c)["mask"], E.reference(c)["labels"]
        assert set(np.unique(m).tolist()) == set(E.WIDE) and 7 not in m
        assert (m[:, 0, 2] == 1).all() and (m[:, 0, 3] == 2 ** 32 + 1).all()                 # they touch
        if c.arg("background") != 2 ** 32 + 1:
            assert (lab[:, 0, 2] != lab[:, 0, 3]).all() and (lab[:, 0, 2] > 0).all() and (lab[:, 0, 3] > 0).all()
    over = _cases("overflow-maps")
    assert {c.arg("max_instances") for c in over} == {1, 7} and all(c.arg("n_maps") == 2 for c in over)
    for c in over:
        ref = E.reference(c)
        assert (ref["count"] > c.arg("max_instances")).all() and ref["labels"].max() > c.arg("max_instances")
        assert (ref["table"][:, :, 7] != 0).all()
    maps = _cases("maps-unaligned")
    assert {c.arg("n_maps") for c in maps} == {1, 2}
    for c in maps:
        assert c.off("map0") % 4 != 0 and c.off("map1") % 4 != 0
        B, H, W = c.shape
        inp, lab = E.inputs(c), E.reference(c)["labels"].reshape(-1)
        for b in range(B):
            edge = -(-(b * H * W + 1) // E.LABEL_SPAN) * E.LABEL_SPAN                          # of the batch's flat pixel index
            assert b * H * W < edge < (b + 1) * H * W and lab[edge - 1] == lab[edge] > 0      # one component through the wave boundary
            inside = lab.reshape(B, H, W)[b] == lab[edge]
            v = inp["map0"][b][inside]
            assert np.isnan(v).any() and (v == 1e9).any() and (v == -1e9).any() and np.isneginf(v).any() and np.isposinf(v).any()
            if "map1" in inp:
                v = inp["map1"][b][inside]
                assert np.isnan(v).any() and (v == -1e9).any() and np.isposinf(v).any()


# ---- run-length masks ----------------------------------------------------------------------------------------------------------------
def test_rle_scan_lengths_classes_and_degenerate_planes():
    rle = [c for c in E.CASES if c.entry == "rle"]
    for n in (1023, 1024, 1025, 2049, 4100):
        (c,) = _cases(f"rle-scan-{n}")
        B, H, W = c.shape
        assert B * len(c.arg("classes")) * W == n and H in (1, 3)
        per_col = np.diff(E.reference(c)["col_offsets"].astype(np.int64))
        assert len(per_col) == n and per_col[:1024].sum() > 0
        if n > E.SCAN_ROUND:
            assert per_col[1024:].sum() > 0 and E.scan_rounds(n) >= 2                        # runs start on both sides of word 1024
    assert {len(c.arg("classes")) for c in rle} >= {1, 8} and {c.shape[1] for c in rle} >= {1, 3}
    assert any(c.shape[2] == 1 for c in rle)
    eight = [c for c in rle if len(c.arg("classes")) == 8][0]
    assert min(eight.arg("classes")) < 0 and 2 ** 32 + 1 in eight.arg("classes") and 1 in eight.arg("classes")
    (c,) = _cases("rle-crossing")
    B, H, W = c.shape
    ref = E.reference(c)
    assert ref["pairs"].tolist() == [[1, H * W]] * B and W > 1                               # one run through every column edge
    for c in rle:
        assert len(E.reference(c)["pairs"]) == E.reference(c)["col_offsets"][-1]


def test_decode_cases():
    dec = [c for c in E.CASES if c.entry == "decode"]
    assert {c.arg("uint8") for c in dec} == {0, 1} and all(c.off("out") % 2 == 1 for c in dec)
    for c in _cases("decode-no-runs"):
        assert len(E.inputs(c)["pairs"]) == 0 and not E.reference(c)["out"].any()
    for c in _cases("decode-empty-segments"):
        o = E.inputs(c)["offsets"].tolist()
        assert o[0] == o[1] == o[2] and o[3] == o[4] == o[5] and o[-1] == o[-2] == o[-3] and o[2] < o[3] < o[6] < o[7]
    for c in _cases("decode-overlap"):
        B, H, W = c.shape
        inp, cl = E.inputs(c), c.arg("classes")
        cov = np.zeros((B, len(cl), H * W), dtype=bool)
        for j in range(B * len(cl)):
            for s0, n in inp["pairs"][inp["offsets"][j]:inp["offsets"][j + 1]]:
                cov[j // len(cl), j % len(cl), s0 - 1:s0 - 1 + n] = True
        both = cov[:, 0] & cov[:, 1]                                                         # covered by both classes: the later one wins
        out = np.stack([o.reshape(-1, order="F") for o in E.reference(c)["out"].astype(np.int64)])
        assert both.any() and (out[both] == cl[1]).all() and (out[cov[:, 0] & ~cov[:, 1]] == cl[0]).all()
        s = inp["pairs"][:, 0]
        assert (np.diff(s[inp["offsets"][0]:inp["offsets"][1]]) < 0).any()                   # unordered
    for c in _cases("decode-clip"):
        B, H, W = c.shape
        assert c.shape == (2, 3, 5)
        p = E.inputs(c)["pairs"].astype(np.int64)
        lo, hi = p[:, 0] - 1, p[:, 0] - 1 + p[:, 1]
        assert lo.min() == -4 and hi.max() == H * W + 4 and (p[:, 0] == 0).any() and (hi > H * W).sum() >= 3
        assert E.reference(c)["out"].any()


# ---- distance transform and surface distances ----------------------------------------------------------------------------------------
def test_surface_class_counts_and_valid_fractions():
    for C in range(1, 9):
        (c,) = _cases(f"col-C{C}")
        assert c.arg("C") == C and c.shape == (2, 37, 53)
        assert S.valid_fraction(E.reference(c)["table"]) >= 0.5, C
    assert {c.pattern for c in _cases("invalid-pairs")} == {"absent", "filled"}
    assert any(S.valid_fraction(E.reference(c)["table"]) < 1.0 for c in _cases("invalid-pairs"))


def test_column_segments():
    seg = [c for c in E.CASES if c.pattern == "segments" and c.entry == "surface"]
    assert {c.shape[1:] for c in seg} == {(H, W) for H in E.SEG_H for W in E.SEG_W}
    assert {E.segments(H)[0] for H in E.SEG_H} == {1, 2, 3, 15, 16}
    assert {W % E.STRIP for W in E.SEG_W} == {2, 0, 1}                                       # the last strip: full, and one lane
    for c in seg:
        _, H, W = c.shape
        nseg, rows = E.segments(H)
        last0 = (nseg - 1) * rows
        for m in E.inputs(c).values():
            for b in range(2):
                ys = {k: np.unique(np.nonzero(m[b] == k)[0]) for k in (1, 2, 3)}
                assert len(ys[1]) and (ys[1] < rows).all()
                assert len(ys[2]) and (ys[2] >= last0).all()
                assert (ys[3] < rows).any() and (ys[3] >= last0).any() and ((ys[3] < rows) | (ys[3] >= last0)).all()
        if H >= 240:
            assert nseg - 2 >= 2                                                             # empty segments between the two
        tab = E.reference(c)["table"]
        assert (tab[:, 1:, 0] > 0).all() and (tab[:, 1:, 1] > 0).all()
    edt = [c for c in E.CASES if c.entry == "edt"]
    assert {(c.shape[1:], c.arg("dtype")) for c in edt} == {((H, W), d) for H in E.SEG_H for W in E.SEG_W for d in (E.U8, E.I32, E.I64)}
    assert all(c.off("mask") % 2 == 1 and c.off("out") % 2 == 1 for c in edt)
    assert E.EDT_VALUE[E.I64] % 2 ** 32 == 0


def test_selection_census_tolerances_scores_and_dtypes():
    sel = _cases("selection")
    assert {c.arg("percentile") for c in sel} == set(E.FRACS)
    seen, n2 = set(), 0
    for c in sel:
        tab = E.reference(c)["table"].reshape(-1, 12)
        for row in tab[(tab[:, 0] > 0) & (tab[:, 1] > 0)]:
            seen.add(E.first_differing_pass(row[10], row[11]))
            n2 += int(row[0] + row[1] == 2)
            if E.first_differing_pass(row[10], row[11]) == 0:
                assert max(row[10], row[11]) >= 256 ** 2
    assert seen == {0, 1, 2, None} and n2 >= len(E.FRACS)
    (c,) = [c for c in sel if c.pattern == "selection" and c.arg("percentile") == 50.0]
    assert E.reference(c)["table"][:, 1, 8:].tolist() == [[1, 2, 1, 90000], [1, 2, 1, 289], [1, 2, 1, 9], [0, 1, 25, 25]]
    tol = _cases("tolerance")
    assert {(c.arg("has_tolerance"), c.arg("tol_d2")) for c in tol} == {(1, 0), (1, 1), (1, 2 ** 25), (0, 9)}
    for c in tol:
        t = E.reference(c)["table"]
        valid = (t[..., 0] > 0) & (t[..., 1] > 0)
        if not c.arg("has_tolerance"):
            assert not t[..., 6:8].any()
        elif c.arg("tol_d2") == 2 ** 25:
            assert np.array_equal(t[..., 6][valid], t[..., 0][valid]) and np.array_equal(t[..., 7][valid], t[..., 1][valid])
        else:
            assert t[..., 6:8].any() and (t[..., 6][valid] < t[..., 0][valid]).any()
    sc = _cases("scores")
    assert {c.arg("C") for c in sc} == {1, 5} and all(c.off("scores") % 4 != 0 for c in sc)
    for c in (c for c in sc if c.arg("C") == 5):
        z, pred = E.inputs(c)["scores"], E.inputs(c)["pred"]
        top = z.max(axis=1, keepdims=True)
        assert ((z == top).sum(axis=1) > 1).mean() > 0.1                                     # ties, the lowest index is the label
        assert np.array_equal(pred, (z == top).argmax(axis=1))
        zero_tie = (top[:, 0] == 0) & (np.signbit(z) & (z == 0)).any(axis=1) & (~np.signbit(z) & (z == 0)).any(axis=1)
        assert zero_tie.any() and np.isposinf(z).any() and np.isneginf(z).any() and not np.isnan(z).any()
    dt = _cases("dtype-pairs")
    assert {(c.arg("pred_dtype"), c.arg("target_dtype")) for c in dt} == {(a, b) for a in (1, 4, 8) for b in (1, 4, 8)}
    for c in dt:
        for side, d in (("pred", c.arg("pred_dtype")), ("target", c.arg("target_dtype"))):
            m = E.inputs(c)[side]
            assert np.array_equal(m.astype(E.NP_OF[d]).astype(np.int64), m) and (m >= c.arg("C")).any() and c.off(side) % 2 == 1
            assert d == E.U8 or (m < 0).any()
        assert S.valid_fraction(E.reference(c)["table"]) == 1.0


# ---- matching ------------------------------------------------------------------------------------------------------------------------
def test_matching_forms_images_and_strides():
    by = {f: _cases(f)[0] for f in ("pair-V4", "pair-V1-pred-off", "pair-V1-target-off", "pair-V1-hw")}
    hw = lambda c: c.shape[1] * c.shape[2]
    v = {f: E.match_v(hw(c), c.off("pred_labels"), c.off("target_labels")) for f, c in by.items()}
    assert v == {"pair-V4": 4, "pair-V1-pred-off": 1, "pair-V1-target-off": 1, "pair-V1-hw": 1} and hw(by["pair-V1-hw"]) % 4 != 0
    same = [by[f] for f in ("pair-V4", "pair-V1-pred-off", "pair-V1-target-off")]
    assert all(E.inputs(c) is not None and all(np.array_equal(E.inputs(c)[k], E.inputs(same[0])[k]) for k in E.inputs(c)) for c in same)
    assert all(c.shape[0] * hw(c) > 2 * E.match_span(4) for c in same) and E.reference(same[0])["pred_out"][..., 3].sum() > 10
    many = _cases("many-images-per-wave")
    assert {c.shape for c in many} == {(70, 2, 2), (50, 1, 3)}
    for c in many:
        V = E.match_v(hw(c), c.off("pred_labels"), c.off("target_labels"))
        assert c.shape[0] * hw(c) <= E.match_span(V) and E.reference(c)["pred_out"][:, 0, 0].astype(bool).sum() >= c.shape[0] // 2
    (c,) = _cases("carry-images")
    assert c.shape == (3, 9, 64) and E.reference(c)["pred_out"][:, 0].tolist() == [[1, 576, 576, 1]] * 3
    assert E.reference(c)["target_out"][:, 0].tolist() == [[1, 576, 576, 1]] * 3
    strides = _cases("matrix-strides")
    assert {(c.arg("max_pred"), c.arg("max_gt")) for c in strides} == set(E.STRIDES)
    for c in strides:
        inp, ref = E.inputs(c), E.reference(c)
        assert (inp["pred_count"] >= 66).all() and (inp["target_count"] >= 131).all()       # past every 64-column group and 32-row round
        mp, mg = c.arg("max_pred"), c.arg("max_gt")
        assert (ref["target_out"][:, mg - 1, 2] > 0).all() and (ref["pred_out"][:, mp - 1, 2] > 0).all()          # the far corner counts
        if mg > 64:                                                                          # counted words in every 64-column group
            assert all((ref["target_out"][:, lo:lo + 64, 2] > 0).any(axis=1).all() for lo in range(0, mg, 64))
        if mp > 32:                                                                          # and in both 32-row rounds
            assert all((ref["pred_out"][:, lo:lo + 32, 2] > 0).any(axis=1).all() for lo in range(0, mp, 32))
            assert (ref["target_out"][..., 0] > 32).any() and (mg == 1 or ((0 < ref["target_out"][..., 0]) & (ref["target_out"][..., 0] <= 32)).any())
        if mg > 64:
            assert all(((ref["pred_out"][..., 0] > lo) & (ref["pred_out"][..., 0] <= lo + 64)).any() for lo in range(64, mg, 64))      # largest intersections there


def test_matching_counts_ties_threshold_and_classes():
    (c,) = _cases("odd-counts")
    inp, ref = E.inputs(c), E.reference(c)
    assert inp["pred_count"][:3].tolist() == [0, -3, 10 ** 6] and inp["target_count"][:3].tolist() == [-1, 10 ** 6, 0]
    assert (inp["pred_labels"] < 0).any() and (inp["target_labels"] == 2 ** 31 - 1).any() and (inp["pred_labels"] > c.arg("max_pred")).any()
    assert not ref["pred_out"][:3].any() and not ref["target_out"][:3].any() and ref["pred_out"][3].any() and ref["counts"][2].any()
    half, threeq = (E.reference(BY) for BY in (E.BY_ID["match-crafted-0.5"], E.BY_ID["match-crafted-0.75"]))
    for ref in (half, threeq):
        assert ref["pred_out"][0, 0, :3].tolist() == [1, 4, 8] and ref["target_out"][0, :, :2].tolist() == [[1, 4], [1, 4]]      # the lower number
        assert ref["target_out"][1, 0, :3].tolist() == [1, 4, 8] and ref["pred_out"][1, :2, :2].tolist() == [[1, 4], [1, 4]]
    tp = E.inputs(E.BY_ID["match-crafted-0.5"])["pred_table"]
    tg = E.inputs(E.BY_ID["match-crafted-0.5"])["target_table"]
    for ref, thr, exact in ((half, 0.5, 2), (threeq, 0.75, 4)):
        inter, union = int(ref["pred_out"][exact, 0, 1]), int(tp[exact, 0, 1] + tg[exact, 0, 1] - ref["pred_out"][exact, 0, 1])
        assert float(inter) == thr * float(union) and ref["pred_out"][exact, 0, 3] == 0 and ref["target_out"][exact, 0, 3] == 0
        assert ref["pred_out"][exact + 1, 0, 1] == inter + 1 and ref["pred_out"][exact + 1, 0, 3] == 1 and ref["target_out"][exact + 1, 0, 3] == 1
    ag = {c.arg("agnostic"): E.reference(c) for c in _cases("agnostic")}
    assert (ag[1]["pred_out"][..., 2] > ag[0]["pred_out"][..., 2]).any()                     # components of different classes overlap
    (c,) = _cases("nc-1")
    assert not E.reference(c)["counts"].any() and E.reference(c)["pred_out"][..., 3].any() and E.reference(c)["counts"].shape == (3, 1, 3)
    (c,) = _cases("nc-64")
    assert E.reference(c)["counts"].shape == (3, 64, 3) and E.reference(c)["counts"][:, 1:4].all()
    (c,) = [c for c in _cases("int64-classes") if c.entry == "match"]
    cls = E.inputs(c)["pred_table"][..., 0]
    assert {-5, 2 ** 32 + 1, 1} <= set(np.unique(cls).tolist()) and E.reference(c)["counts"][:, 1, 1:].all() and not E.reference(c)["counts"][:, 2:].any()
    dense, sparse = E.BY_ID[E.STALE[0]], E.BY_ID[E.STALE[1]]
    assert dense.shape[0] == sparse.shape[0] and sparse.arg("max_pred") * sparse.arg("max_gt") < dense.arg("max_pred") * dense.arg("max_gt")


# ---- the comparison rejects planted mistakes -----------------------------------------------------------------------------------------
def _copy(ref):
    return {k: v.copy() for k, v in ref.items()}


def test_the_comparison_accepts_the_reference_and_rejects_planted_mistakes():
    for c in (E.BY_ID[i] for i in ("label-carry-9x64-full", "rle-scan-2049", "surf-select-50", "match-crafted-0.5", "decode-clip-i64")):
        assert E.compare(E.reference(c), _copy(E.reference(c))) == []
    # an area moved between two images' first components
    c = E.BY_ID["label-carry-9x64-full"]
    g = _copy(E.reference(c))
    g["table"][0, 0, 1] += g["table"][1, 0, 1]
    g["table"][1, 0, 1] = 0
    assert E.compare(E.reference(c), g)
    # a scan carry dropped after word 1024: the numbering of an image starts again there, the run offsets likewise
    c = E.BY_ID["label-scan-min1"]
    ref = E.reference(c)
    g = _copy(ref)
    for b in range(c.shape[0]):
        first = ref["table"][b, :ref["count"][b], 6]
        before = int((first < 1024 * E.CHUNK).sum())
        lab = g["labels"][b]
        lab[lab > before] -= before
    assert E.compare(ref, g) and not [m for m in E.compare(ref, g) if not m.startswith("labels")]
    c = E.BY_ID["rle-scan-2049"]
    g = _copy(E.reference(c))
    g["col_offsets"][1024:] -= g["col_offsets"][1024]
    assert E.compare(E.reference(c), g)
    # classes compared modulo 2^32
    c = E.BY_ID["label-wide-bg-m5"]
    lab, cnt, tab = I.label_batch(E.inputs(c)["mask"] % 2 ** 32, (), 4, (-5) % 2 ** 32, 1, c.arg("max_instances"))
    assert E.compare(E.reference(c), dict(labels=lab, count=cnt, table=E.reference(c)["table"]))
    c = [c for c in E.CASES if c.entry == "match" and c.arg("wide_classes")][0]
    inp = E.inputs(c)
    narrow = M.match_batch((inp["pred_labels"], inp["pred_count"], inp["pred_table"] % 2 ** 32),
                           (inp["target_labels"], inp["target_count"], inp["target_table"] % 2 ** 32), 4)
    assert E.compare(E.reference(c), dict(pred_out=narrow[0], target_out=narrow[1], counts=E.reference(c)["counts"]))
    for dtype_case in ("surf-dtype-8-8", "surf-dtype-8-4"):
        c = E.BY_ID[dtype_case]
        inp = E.inputs(c)
        low = lambda m: m.astype(np.int32).astype(np.int64)
        assert E.compare(E.reference(c), dict(table=S.table(low(inp["pred"]), inp["target"], c.arg("C"))))
    # a rank taken one too low
    c = E.BY_ID["surf-select-50"]
    g = _copy(E.reference(c))
    g["table"][0, 1, 11] = g["table"][0, 1, 10]
    assert E.compare(E.reference(c), g)
    # a tie resolved to the higher number
    c = E.BY_ID["match-crafted-0.5"]
    g = _copy(E.reference(c))
    g["pred_out"][0, 0, 0] = 2
    assert E.compare(E.reference(c), g)
    # one matrix word left stale: its value in `covered`
    g = _copy(E.reference(c))
    g["target_out"][1, 0, 2] += 0x7F7F7F7F
    assert E.compare(E.reference(c), g)
    # a decode without its clip: a run's overshoot lands on a pixel of the plane
    c = E.BY_ID["decode-clip-i64"]
    g = _copy(E.reference(c))
    assert g["out"][0, 0, 1] == 0
    g["out"][0, 0, 1] = c.arg("classes")[0]
    assert E.compare(E.reference(c), g)
    # wrong types and shapes
    assert E.compare(E.reference(c), dict(out=E.reference(c)["out"].astype(np.float64)))
    assert E.compare(E.reference(c), dict(out=E.reference(c)["out"][:1])) and E.compare(E.reference(c), {})
