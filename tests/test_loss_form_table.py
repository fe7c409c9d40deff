"""The loss-block table of tests/loss_ref.py on the CPU: the table covers every (D, C) in every form, the restated dispatch gives the
forms it should, the seeded inputs keep their pseudo-labels clear of ties, the reference's scalar blocks and closed form agree with
the oracle, and the bars of tests/test_gpu_loss_forms.py reject a set of subtle mistakes planted in the reference's own outputs."""
import numpy as np
import pytest
import torch

import loss_ref as R
from oracle import uaps_oracle as O


def test_ids_are_unique_and_every_dc_appears_in_every_form():
    ids = [c.id for c in R.CASES]
    assert len(ids) == len(set(ids))
    assert len(R.ALL_DC) == 56
    for D, C in R.ALL_DC:
        V = R.unsup_vec(D, C)
        pair = {(c.form_sup, c.form, c.track) for c in R.PAIR_GROUPS[(D, C)] if c.entry == R.PAIR and (c.D, c.C) == (D, C)}
        wide = "scalar" if V == 1 else f"vec{V}"
        assert pair == {("vec4", wide, True), ("vec4", wide, False), ("scalar", "scalar", True), ("scalar", "scalar", False)}, (D, C, pair)
        two = {(c.form_sup, c.form) for c in R.TWO_GROUPS[(D, C)] if c.entry == R.TWO_BRANCH and (c.D, c.C) == (D, C)}
        assert ("vec4", wide) in two and ("scalar", "scalar") in two, (D, C, two)
        if 16 < D * C <= 32:
            assert ("scalar", "vec2") in two, (D, C, two)              # H*W % 4 == 2: V = 2 for the unsupervised kernels only
    assert sum(len(g) for g in R.PAIR_GROUPS.values()) == 224
    # the data two runs share differs in nothing but what must not change the bits
    for g in R.PAIR_GROUPS.values():
        assert g[0].seed_id == g[1].seed_id != g[2].seed_id == g[3].seed_id
        assert {c.want_var for c in g[:2]} != {c.want_var for c in g[2:]}
    assert {c.want_var for g in R.PAIR_GROUPS.values() for c in g} == {True, False}


def test_shapes_split_into_the_blocks_the_table_is_built_for():
    v, s, v2 = (R.Case("s", R.PAIR, 4, *sh[:1], 4, *sh[1:]) for sh in (R.VEC_SHAPE, R.SCALAR_SHAPE, R.V2_SHAPE))
    assert (v.HW, v.N, v.blocks(4), v.blocks(2), v.blocks(1)) == (720, 2160, 3, 5, 9) and (v.N // 4) % R.THREADS != 0
    assert (s.HW, s.N, s.blocks(1)) == (221, 663, 3) and s.N % R.THREADS != 0
    assert v2.HW == 126 and v2.HW % 4 == 2
    assert any(b * v.HW % (4 * R.THREADS) for b in range(1, v.B))          # an image boundary inside a block


@pytest.mark.parametrize("kw,sup,unsup", [
    (dict(entry=R.PAIR, D=4, C=4, H=20, W=36), "vec4", "vec4"),
    (dict(entry=R.PAIR, D=6, C=4, H=20, W=36), "vec4", "vec2"),
    (dict(entry=R.PAIR, D=8, C=8, H=20, W=36), "vec4", "scalar"),
    (dict(entry=R.PAIR, D=4, C=4, H=13, W=17), "scalar", "scalar"),
    (dict(entry=R.PAIR, D=5, C=5, H=9, W=14), "scalar", "scalar"),             # H*W % 4 == 2: the pair kernels have no V = 2 route
    (dict(entry=R.PAIR, D=4, C=4, H=20, W=36, off=1), "scalar", "scalar"),
    (dict(entry=R.PAIR, D=4, C=4, H=20, W=36, lab_off=1), "scalar", "scalar"),
    (dict(entry=R.PAIR, D=4, C=4, H=20, W=36, lab_off=2), "vec4", "vec4"),
    (dict(entry=R.SUMS, D=3, C=5, H=20, W=36), "vec4", "vec4"),
    (dict(entry=R.TWO_BRANCH, D=5, C=5, H=9, W=14), "scalar", "vec2"),
    (dict(entry=R.TWO_BRANCH, D=4, C=4, H=9, W=14), "scalar", "scalar"),
    (dict(entry=R.TWO_BRANCH, D=5, C=5, H=9, W=14, off=1), "scalar", "scalar"),
    (dict(entry=R.TWO_BRANCH, D=7, C=8, H=20, W=36), "vec4", "scalar"),
    (dict(entry=R.TWO_BRANCH, D=2, C=8, H=1, W=4), "vec4", "vec4")])
def test_form_restatement(kw, sup, unsup):
    c = R.Case("t", B=2, **kw)
    assert (c.form_sup, c.form) == (sup, unsup)


def test_kernel_names():
    assert R.BY_ID["pair-6x4-vec-track"].kernels == ("pair_fwd_kernel<6, 4, 4, 2, false, false, 2>", "pair_bwd_kernel<6, 4, 4, 2, true>")
    assert R.BY_ID["pair-3x5-scalar-plain"].kernels == ("pair_fwd_kernel<3, 5, 1, 1, false, false, 2>", "pair_bwd_kernel<3, 5, 1, 1, true>")
    assert R.BY_ID["two-5x5-v2"].kernels == ("unsup_fwd_kernel<5, 5, 2>", "unsup_bwd_kernel<5, 5, 2>", "sup_fwd_kernel<5, 5, 1>", "sup_bwd_kernel<5, 5, 1>")
    for dc in R.EXTRA_DC:
        forms = {c.id.split("-", 2)[2]: c.form_sup for c in R.EXTRA_GROUPS[dc]}
        assert forms["off1"] == forms["laboff1"] == forms["tiny-2x1x1"] == "scalar" and forms["base"] == forms["tiny-1x1x4"] == forms["b1"] == "vec4"


def test_every_case_keeps_its_pseudo_labels_clear_of_ties():
    """From the float64 reference alone: at most TIE_SHARE of a case's pixels may have a top-two margin below MARGIN (planted ties
    apart), and every planted tie is an exact tie between its two classes, ahead of the rest."""
    seen = set()
    for case in R.CASES:
        key = (case.seed_id or case.id)
        if key in seen:
            continue
        seen.add(key)
        inp = R.inputs(case)
        am, margin = R.margin_and_argmax(inp)
        close = margin.reshape(-1) < R.MARGIN
        if case.planted == "ties":
            assert np.all(margin.reshape(-1)[inp["planted"]] == 0.0), case.id
            assert np.array_equal(am.reshape(-1)[inp["planted"]], inp["tie_class"]), case.id
            close[inp["planted"]] = False
        assert close.sum() <= R.TIE_SHARE * case.N, (case.id, int(close.sum()))
        assert all(a.dtype == np.float32 and np.all(np.isfinite(a)) for a in inp["lab"] + inp["un"])


SELF_TEST = ("x-4x4-base", "x-3x5-nloss2", "pair-6x3-vec-track")


@pytest.fixture(scope="module", params=SELF_TEST)
def refd(request):
    case = R.BY_ID[request.param]
    inp = R.inputs(case)
    return case, inp, R.full_reference(case, inp)


def test_scalar_blocks_and_closed_form_agree_with_the_oracle(refd):
    """slots() restates the finalize arithmetic from the oracle's raw sums: its named values must be the oracle's own
    (step_loss for one rank); closed_form_grads() must be the oracle's autograd gradient."""
    case, inp, ref = refd
    D, C = case.D, case.C
    ul, sl, S = R.u_layout(D, C), R.s_layout(D, C), ref["slots"]
    for name in ("ps_loss", "l_uncert"):
        np.testing.assert_allclose(R.slot(S["u"], ul, name)[0], ref[name], rtol=1e-12)
    np.testing.assert_allclose(R.slot(S["s"], sl, "sup")[0], ref["sup"], rtol=1e-12)
    np.testing.assert_allclose(R.slot(S["u"], ul, "total")[0], ref["loss"], rtol=1e-12)          # the oracle's loss is the step's total
    np.testing.assert_allclose(R.slot(S["u"], ul, "loss")[0], ref["loss"] - ref["sup"], rtol=1e-11)
    if case.nloss_mult == 1:
        t = lambda a: torch.tensor(a, dtype=torch.float64)
        o = O.step_loss([t(a) for a in inp["un"]], [t(a) for a in inp["lab"]], torch.tensor(inp["labels"]),
                        [float(np.float32(x)) for x in inp["w"]], inp["cw1"], inp["cw2"])
        np.testing.assert_allclose(R.slot(S["u"], ul, "ce"), [float(v) for v in o["ce"]], rtol=1e-12)
        np.testing.assert_allclose(R.slot(S["u"], ul, "s"), [float(v) for v in o["s"]], rtol=1e-9)      # (eps: 1e-7 there, its fp32 value here)
        np.testing.assert_allclose(R.slot(S["u"], ul, "E"), [float(v.mean()) for v in o["evar"]], rtol=1e-12)
        np.testing.assert_allclose(R.slot(S["s"], sl, "ce"), [float(v) for v in o["ce_sup"]], rtol=1e-12)
        np.testing.assert_allclose(R.slot(S["s"], sl, "dice"), [float(v) for v in o["dice_sup"]], rtol=1e-9)
        np.testing.assert_allclose(ref["var"], torch.stack(o["var"]).numpy(), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(ref["q"]["u"]["v"].reshape(ref["var"].shape), ref["var"], rtol=1e-10, atol=1e-13)
    dl, du = R.closed_form_grads(case, inp, ref["q"], S)
    assert np.abs(dl - ref["dlab"]).max() <= 1e-12 * np.abs(ref["dlab"]).max()
    assert np.abs(du - ref["dun"]).max() <= 1e-12 * np.abs(ref["dun"]).max()
    assert R.ratio(dl, ref["dlab"], ref["c_dlab"]) < 1e-14 and R.ratio(du, ref["dun"], ref["c_dun"]) < 1e-14


def _flagged(case, inp, ref, got):
    ratios, bad = R.compare(case, inp, ref, got)
    return bool(bad) or bool(R.over_bars(ratios))


def test_the_bars_catch_planted_mistakes(refd):
    """The reference's own outputs rounded to fp32 pass; each planted mistake is flagged under the final TAU."""
    case, inp, ref = refd
    D, C, N = case.D, case.C, case.N
    ul = R.u_layout(D, C)
    f32 = lambda a: np.asarray(a, np.float32)
    clean = lambda: R.as_got(case, inp, ref)
    ratios, bad = R.compare(case, inp, ref, clean())
    assert not bad and not R.over_bars(ratios), (ratios, bad)
    assert all(v < 0.2 * R.TAU[k] for k, v in ratios.items()), ratios               # fp32 rounding alone sits far inside every bar
    # the last vector group of one head left unwritten
    g = clean()
    g["dun"][D - 1].reshape(-1)[-4:] = np.nan
    assert _flagged(case, inp, ref, g)
    g = clean()
    g["dlab"][0].reshape(-1)[-4:] = 0.0                                              # ... or written as zeros
    assert _flagged(case, inp, ref, g)
    # 1 / N where 1 / Nloss belongs (visible when the loss runs over more pixels than the launch)
    if case.nloss_mult > 1:
        g = clean()
        dl, du = R.closed_form_grads(case, inp, ref["q"], ref["slots"], n_ce=N)
        g["dlab"], g["dun"] = f32(dl), f32(du)
        assert _flagged(case, inp, ref, g)
        g = clean()
        g["dun"] = f32(du)
        assert _flagged(case, inp, ref, g)
    # a1 and a2 swapped
    g = clean()
    (o1, n), (o2, _) = ul["a1"], ul["a2"]
    g["uscal"][o1:o1 + n], g["uscal"][o2:o2 + n] = g["uscal"][o2:o2 + n].copy(), g["uscal"][o1:o1 + n].copy()
    assert _flagged(case, inp, ref, g)
    # one head's weight (its 1 / D share of the pseudo-supervision term) off by 1e-4 relative: in its gradient, and in ps_loss alone
    hw = np.ones(D)
    hw[D // 2] += 1e-4
    g = clean()
    g["dun"] = f32(R.closed_form_grads(case, inp, ref["q"], ref["slots"], head_w=hw)[1])
    assert _flagged(case, inp, ref, g)
    g = clean()
    s, E = R.slot(ref["slots"]["u"], ul, "s"), R.slot(ref["slots"]["u"], ul, "E")
    g["uscal"][ul["ps_loss"][0]] = np.float32((s * E * hw).mean())
    assert _flagged(case, inp, ref, g)
    # a gradient scaled by 1 / D twice
    g = clean()
    g["dun"] = f32(R.closed_form_grads(case, inp, ref["q"], ref["slots"], extra_div=True)[1])
    assert _flagged(case, inp, ref, g)
    # an amax that misses the odd-index classes
    g = clean()
    even = float(max(np.abs(g["dlab"][:, :, 0::2]).max(), np.abs(g["dun"][:, :, 0::2]).max()))
    if case.track and even != g["amax"]:
        g["amax"] = even
        assert _flagged(case, inp, ref, g)
    # a pseudo-label off at one clear pixel, a count off by one
    g = clean()
    i = int(np.argmax(ref["margin"].reshape(-1)))
    g["pseudo"].reshape(-1)[i] = (g["pseudo"].reshape(-1)[i] + 1) % C
    assert _flagged(case, inp, ref, g)
    g = clean()
    g["uscal"][ul["cnt"][0]] += 1
    assert _flagged(case, inp, ref, g)


def test_the_odd_class_amax_mistake_is_visible_in_the_self_test_cases():
    """(the previous test plants it only where it changes the value: at least one tracked case must have its maximum on an odd class)"""
    hit = 0
    for cid in SELF_TEST:
        case = R.BY_ID[cid]
        if not case.track:
            continue
        inp = R.inputs(case)
        g = R.as_got(case, inp, R.full_reference(case, inp))
        hit += float(max(np.abs(g["dlab"][:, :, 0::2]).max(), np.abs(g["dun"][:, :, 0::2]).max())) != g["amax"]
    assert hit >= 1
