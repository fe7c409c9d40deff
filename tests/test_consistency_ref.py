"""The references of tests/consistency_ref.py on the CPU: every reference against torch in float64 (softmax, F.kl_div, torch.rot90 and
autograd of the plain formulas the kernels' comments quote), the EMA restatement against exact rational arithmetic, the comparison code
of tests/test_gpu_consistency_forms.py passing the unmutated references and rejecting every mutant, the ambiguity and clamp-edge caps
on every case, and the case table naming exactly the kernels of loss_mean_teacher.hip, loss_cct_dct.hip and the first half of
pair_ops.hip that the built code object holds."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import consistency_ref as R
from ops_ref import words
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


# ---- bit-exact restatements -------------------------------------------------------------------------------------------------------
def test_ema_is_the_twice_rounded_fma_exactly():
    """fma(oma, p, rn(e alpha)) against exact rationals, on random data, on a constructed double-rounding trap and at step 0."""
    rng = np.random.default_rng(5)
    e, p = rng.standard_normal(400).astype(F32), rng.standard_normal(400).astype(F32)
    # the trap: oma p + m lies just above a float32 midpoint, by less than float64 resolves: a float64 sum rounds it onto the tie
    e[0], p[0] = F32(1.0), F32(2.0 ** -30)
    for a, oma in ((0.99, 0.01), (0.5, 0.5), (0.0, 1.0), (1.0 + 2.0 ** -23, 1.0 + 2.0 ** -23)):
        a32, o32 = F32(a), F32(oma)
        got = R.ema(e, p, a32, o32)
        once = R.ema(e, p, a32, o32, "round_once")

        def rn(fr):                           # exact rational -> nearest float32, ties to even
            f = F32(float(fr))                # float(Fraction) is correctly rounded; re-round by hand when that landed on a tie
            lo, hi = np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf))
            best = min((abs(Fraction(float(c)) - fr), int(np.array(c, F32).view(np.uint32)) & 1, float(c)) for c in (lo, f, hi))
            return F32(best[2])
        for i in range(0, 400, 7):
            m = rn(Fraction(float(e[i])) * Fraction(float(a32)))
            assert got[i] == rn(Fraction(float(o32)) * Fraction(float(p[i])) + Fraction(float(m))), (a, i)
            assert once[i] == rn(Fraction(float(o32)) * Fraction(float(p[i])) + Fraction(float(e[i])) * Fraction(float(a32))), (a, i)
    assert np.array_equal(R.ema(e, p, 0.0, 1.0), p)                  # step 0: a bit copy
    assert R.ema_alpha(0.99, 0) == (0.0, 1.0) and R.ema_alpha(0.99, 1) == (0.5, 0.5) and R.ema_alpha(0.99, 10 ** 6)[0] == 0.99


def test_rn32_sum_rounds_once():
    """1 + 2^-24 + 2^-60: float64 rounds the sum to the float32 tie 1 + 2^-24 (-> 1.0, even); rounded once it is 1 + 2^-23."""
    assert F32(F64(1.0 + 2.0 ** -24) + 2.0 ** -60) == F32(1.0)
    assert R._rn32_sum(np.array([1.0 + 2.0 ** -24]), np.array([2.0 ** -60]))[0] == F32(1.0 + 2.0 ** -23)
    assert R._rn32_sum(np.array([1.0 + 2.0 ** -24]), np.array([-2.0 ** -60]))[0] == F32(1.0)
    assert R._rn32_sum(np.array([1.0 + 2.0 ** -24]), np.array([0.0]))[0] == F32(1.0)


def test_noise_apply_matches_torch():
    c, inp, ref = _ref("apply-T3")
    B = c.shape[0]
    x, n = torch.from_numpy(inp["x"]), torch.from_numpy(inp["noise"]).reshape((4 * B,) + c.shape[1:])
    want = x.repeat(4, 1, 1, 1) + torch.clamp(n * 0.1, -0.2, 0.2)
    assert R.bits_differ(ref.exact["out"], want.numpy()) == 0
    assert (np.abs(inp["noise"] * 0.1) > 0.2).mean() > 0.1            # the clamp is at work


def test_noise_draw_layout_and_moments():
    """Element i: counter offset + i / 4; words 0, 1 -> Box-Muller pair (cos, sin) = elements 0, 1; words 2, 3 -> elements 2, 3."""
    seed, off = 0xFEDCBA9876543210, 2 ** 32 - 2
    g = R.gauss_E(seed, off, 11)
    for i in (0, 1, 2, 3, 6, 9, 10):
        w = words(seed, np.array([off + i // 4], np.uint64))[0]
        a, b = (int(w[0]), int(w[1])) if i % 4 < 2 else (int(w[2]), int(w[3]))
        rad = np.sqrt(-2 * np.log(((a >> 8) + 1) * 2.0 ** -24))
        ang = 2 * np.pi * ((b >> 8) * 2.0 ** -24)
        assert abs(g.v[i] - rad * (np.cos(ang), np.sin(ang))[i % 2]) <= 1e-12, i
    big = R.gauss_E(seed, 0, 1 << 16)
    assert abs(big.v.mean()) < 0.02 and abs(big.v.std() - 1) < 0.02 and big.e.max() < 4e-5 and np.abs(big.v).max() <= 5.77
    val, bar, edge = R.noise_draw(np.zeros((1, 1, 256, 256), F32), 1, 0, seed, 0)
    assert np.abs(val).max() <= float(R.C02) and 0.03 < (np.abs(val) == float(R.C02)).mean() < 0.06 and edge <= 65   # |n| > 2: 4.55 %


@pytest.mark.parametrize("k", range(4))
def test_rot90_matches_torch(k):
    x = np.random.default_rng(k).standard_normal((2, 3, 5, 9)).astype(F32)
    assert np.array_equal(R.rot90(x, k), torch.rot90(torch.from_numpy(x), k, [2, 3]).numpy())
    ref = R.rot90_batch(x, 2 * x, k, 0.5)
    assert ref.exact["amax"] == float(np.abs(2 * x).max()) and ref.exact["cat"].size == 2 * x.size


# ---- the float64 references against torch autograd --------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["mt-c3", "mt-c6", "mt-sat"])
def test_mt_matches_torch(cid):
    c, inp, ref = _ref(cid)
    s = _t(inp["s"], True)
    loss = ((torch.softmax(s, 1) - torch.softmax(_t(inp["e"]), 1)) ** 2).mean()              # MT_train.py:199
    _close(ref.f64["loss"][0], loss)
    (c.g * loss).backward()
    cb = R.Case("b", "mc_bwd", shape=c.shape, mode="mt")
    _close(R.reference(cb, inp).f64["ds"][0], s.grad)


@pytest.mark.parametrize("cid", ["uamt-3x33x45-T3", "uamt-c2-T0", "uamt-3x33x45-T16", "uamt-2x16x24-T1"])
def test_uamt_matches_torch(cid):
    c, inp, ref = _ref(cid)
    s, e, mc = _t(inp["s"], True), _t(inp["e"]), _t(inp["mc"])
    pb = torch.softmax(mc, 2).mean(0) if c.T > 0 else mc                                       # UA_MT_train.py:194-200
    unc = -(pb * torch.log(pb + R.EPS6)).sum(1)
    _close(ref.f64["unc"][0] if c.unc else R.mc_uncertainty(inp["mc"], c.T).v, unc)
    mask = (unc < inp["thr"]).double()
    dist = ((torch.softmax(s, 1) - torch.softmax(e, 1)) ** 2).sum(1)
    loss = (mask * dist).sum() / (2 * mask.sum() + 1e-16)                                    # UA_MT_train.py:212-214
    got = R.as_got(ref)
    assert np.array_equal(got["mask"], mask.numpy().astype(np.uint8)) and got["sum_m"] == F32(mask.sum().item())
    _close(ref.f64["loss"][0], loss)
    (c.g * loss).backward()
    cb = R.Case("b", "mc_bwd", shape=c.shape, mode="mask")
    _close(R.reference(cb, dict(inp, mask=got["mask"], sum_m=float(mask.sum()))).f64["ds"][0], s.grad)
    assert 0 < mask.mean() < 1


@pytest.mark.parametrize("cid", ["cct-c3-v4", "cct-c4-v1", "cct-c2-forced", "cct-sat"])
def test_cct_matches_torch(cid):
    c, inp, ref = _ref(cid)
    B = c.shape[0]
    hs = [_t(h, True) for h in inp["heads"]]
    ps = [torch.softmax(h[c.b0:c.b0 + B], 1) for h in hs]
    terms = [((ps[0] - p) ** 2) for p in ps[1:]]
    loss = sum(t.mean() for t in terms) / (c.D - 1)                                          # CCT_train.py:195-200
    _close(ref.f64["loss"][0], loss)
    _close(ref.f64["sums"][0], np.array([t.sum().item() for t in terms]))
    (c.g * loss).backward()
    cb = R.Case("b", "cct_bwd", shape=c.shape, D=c.D, b0=c.b0, Btot=c.Btot)
    rb = R.reference(cb, inp)
    for k, h in enumerate(hs):
        _close(rb.f64[f"dz{k}"][0], h.grad[c.b0:c.b0 + B], scale=float(h.grad.abs().max()))
        out = torch.ones(h.shape[0], dtype=torch.bool)
        out[c.b0:c.b0 + B] = False
        assert not h.grad[out].any()


@pytest.mark.parametrize("cid", ["rot-k0", "rot-k1", "rot-k2", "rot-k3", "rot-c3", "rot-c6", "rot-shift"])
def test_rot_consistency_matches_torch(cid):
    c, inp, ref = _ref(cid)
    B = c.shape[0]
    r, u = _t(inp["r"], True), _t(inp["u"], True)
    loss = ((torch.softmax(r[c.r_b0:c.r_b0 + B], 1) - torch.rot90(torch.softmax(u[c.u_b0:c.u_b0 + B], 1), c.k, [2, 3])) ** 2).mean()
    _close(ref.f64["loss"][0], loss)                                                         # DCT_train.py:188
    (c.g * loss).backward()
    cb = R.Case("b", "rot_bwd", shape=c.shape, k=c.k, r_b0=c.r_b0, u_b0=c.u_b0, r_tot=c.r_tot, u_tot=c.u_tot)
    rb = R.reference(cb, inp)
    _close(rb.f64["dr"][0], r.grad[c.r_b0:c.r_b0 + B])
    _close(rb.f64["du"][0], u.grad[c.u_b0:c.u_b0 + B])


@pytest.mark.parametrize("cid", ["pair-randn2", "pair-sat", "pair-equal", "pair-shift", "pair-c3", "pair-outs6"])
def test_pair_fwd_matches_torch(cid):
    c, inp, ref = _ref(cid)
    a, b = _t(inp["a"], True), _t(inp["b"], True)
    pa, pb = torch.softmax(a, 1), torch.softmax(b, 1)
    _close(ref.f64["mse_map"][0], (pa - pb) ** 2)                                            # losses_1.py:9-26
    kl = F.kl_div(torch.log_softmax(a, 1), pb, reduction="none")
    scale = 1e4 if c.regime == "shift" else None             # float64 itself loses 1e4 x 2^-53 where the logits carry the shift
    _close(ref.f64["kl_map"][0], kl.sum(1), scale)
    _close(ref.f64["kl_mean"][0], F.kl_div(torch.log_softmax(a, 1), pb, reduction="mean"), scale)   # losses_1.py:29-48
    if c.regime == "shift":
        return
    # the three backward entry points on the same tensors
    g = torch.from_numpy(np.random.default_rng(1).standard_normal(c.shape))
    da, = torch.autograd.grad((g * (pa - pb.detach()) ** 2).sum(), a, retain_graph=True)
    _close(R.mse_bwd(inp["a"], inp["b"], g.numpy().astype(F32)).f64["da"][0], torch.autograd.grad(
        (_t(g.numpy().astype(F32)) * (pa - pb.detach()) ** 2).sum(), a, retain_graph=True)[0], scale=float(da.abs().max()) + 1e-30)
    da, = torch.autograd.grad(0.75 * F.kl_div(torch.log_softmax(a, 1), pb.detach(), reduction="mean"), a, retain_graph=True)
    _close(R.kl_bwd(inp["a"], inp["b"], 0.75).f64["da"][0], da)
    _close(R.kl_bwd(inp["a"], inp["b"], None).f64["da"][0], da / 0.75)
    gm = np.random.default_rng(2).standard_normal((c.shape[0],) + c.shape[2:]).astype(F32)
    da, db = torch.autograd.grad((_t(gm) * kl.sum(1)).sum(), (a, b))                         # UCC_train.py:213-217: nothing detached
    rk = R.klmap_bwd(inp["a"], inp["b"], gm)
    _close(rk.f64["da"][0], da)
    _close(rk.f64["db"][0], db, scale=float(db.abs().max()) + 1e-30)


@pytest.mark.parametrize("cid", ["pairp-c4", "pairp-01", "pairp-01-map"])
def test_pair_probs_matches_torch_and_its_non_finite_kinds(cid):
    c, inp, _ = _ref(cid)
    ref = R.pair_fwd(inp["a"], inp["b"], True)
    pr, gt = _t(inp["a"]), _t(inp["b"])
    kl = F.kl_div(torch.log(pr), gt, reduction="none").sum(1).numpy()                        # losses_2.py:201-213
    assert np.array_equal(R.kinds(kl), ref.nonfinite)
    fin = ref.nonfinite == 0
    _close(ref.f64["kl_map"][0][fin], kl[fin])
    if cid == "pairp-c4":
        _close(ref.f64["kl_mean"][0], F.kl_div(torch.log(pr), gt, reduction="mean"))
    else:
        assert "kl_mean" not in ref.f64 and {0, 1, 3} <= set(np.unique(ref.nonfinite).tolist())
        assert (inp["a"] == 0).any() and (inp["a"] == 1).any() and (inp["b"] == 0).any() and (inp["b"] == 1).any()


@pytest.mark.parametrize("cid", ["ent-c2", "ent-c5", "ent-01"])
def test_entropy_matches_torch(cid):
    c, inp, ref = _ref(cid)
    p = _t(inp["p"])
    ent = -(p * torch.log(p + R.EPS6)).sum(1)                                                # losses_1.py:139-149
    _close(ref.f64["ent_map"][0], ent)
    _close(ref.f64["ent_mean"][0], ent.mean())


def test_regimes_are_what_they_say():
    rng = np.random.default_rng(0)
    sat = R.logits(rng, (2, 4, 16, 24), "sat").astype(F64)
    p = np.exp(sat - sat.max(1, keepdims=True))
    assert (p.astype(F32) == 0).mean() > 0.05                         # exponentials underflow in float32
    eq = R.logits(rng, (2, 4, 16, 24), "equal")
    assert (eq == eq[:, :1]).all() and np.unique(eq).size > 100
    sh = R.logits(rng, (2, 4, 16, 24), "shift")
    assert sh.min() > 9980 and np.unique(sh - F32(1e4)).size > 100
    pr = R.probabilities(rng, (2, 4, 16, 24), "probs")
    assert pr.min() > 1e-30 and np.abs(pr.sum(1) - 1).max() < 1e-6   # no denormal inputs: v_log_f32 alone would flush them


# ---- the comparison passes the references and rejects the mutants -----------------------------------------------------------------
def _self_compare(c, mut=""):
    inp = R.inputs(c)
    ref = R.reference(c, inp)
    got, bad0 = R.window_split(ref, R.as_full(R.reference(c, inp, mut) if mut else ref, c, inp))
    ratios, bad = R.compare(ref, got)
    return ratios, bad0 + bad, ref


@pytest.mark.parametrize("entry", R.ENTRIES)
def test_comparison_passes_every_reference_and_the_caps_hold(entry):
    """as_got rounds the float64 values to float32: inside every bar.  R.reference asserts the ambiguity and clamp-edge caps."""
    for c in (c for c in R.CASES if c.entry == entry):
        ratios, bad, ref = _self_compare(c)
        assert not bad, (c.id, bad)
        assert ref.exact or ref.f64, c.id
        for k, (val, bar) in ref.f64.items():
            assert np.all(np.asarray(bar) >= 0) and np.all(np.isfinite(bar)) and np.all(np.isfinite(val)), (c.id, k)


MUTANTS = [
    ("denom_m", "uamt-3x33x45-T3"), ("denom_m", "uamt-cap"), ("denom_m", "uamtb-c3"),
    ("nc_vs_n", "mt-c2"), ("nc_vs_n", "mtb-c7"), ("nc_vs_n", "pair-c8"), ("nc_vs_n", "pairp-c4"),
    ("d_vs_dm1", "cct-c3-v4"), ("d_vs_dm1", "cct-c4-v1"), ("d_vs_dm1", "cctb-c2-v4"), ("d_vs_dm1", "cctb-c6-forced"),
    ("t_sum", "uamt-3x33x45-T3"), ("t_sum", "uamt-3x33x45-T16"),
    ("no_eps", "uamt-sat"), ("no_eps", "uamt-c2-T0"), ("no_eps", "ent-01"), ("no_eps", "ent-c3"),
    ("head0_no_sum", "cctb-c3-v4"), ("head0_no_sum", "cctb-c3-v1"),
    ("du_detached", "rotb-c2"), ("du_detached", "rotb-k2"),
    ("k_swap", "rot-k1"), ("k_swap", "rot-k3"), ("k_swap", "rotb-k1"), ("k_swap", "rotb-k3"), ("k_swap", "rot90-k1"), ("k_swap", "rot90-k3"),
    ("k_swap", "rot90-k1-sq"), ("k_swap", "rot-cap-k1"),
    ("window_ignored", "cct-c3-v4"), ("window_ignored", "cctb-c2-v4"), ("window_ignored", "cctb-c3-v1"), ("window_ignored", "rot-c3"),
    ("window_ignored", "rotb-c2"),
    ("target_grad", "klb-c4"), ("target_grad", "klb-sat"), ("target_detached", "klmapb-c2"),
    ("word_rot", "noise-T1"), ("word_rot", "noise-offo"), ("ctr_shift", "noise-T0"), ("ctr_shift", "noise-T16"),
    ("round_once", "ema-n128"), ("round_once", "ema-sizes"), ("round_once", "ema-late")]


@pytest.mark.parametrize("mut,cid", MUTANTS)
def test_comparison_rejects_mutant(mut, cid):
    ratios, bad, _ = _self_compare(R.BY_ID[cid], mut)
    assert bad, (mut, cid, ratios)


def test_every_listed_mutant_is_tried():
    assert {m for m, _ in MUTANTS} == {"denom_m", "nc_vs_n", "d_vs_dm1", "t_sum", "no_eps", "head0_no_sum", "du_detached", "k_swap",
                                       "window_ignored", "target_grad", "target_detached", "word_rot", "ctr_shift", "round_once"}


def test_a_wrong_mask_bit_outside_the_ambiguous_band_is_rejected():
    c = R.BY_ID["uamt-3x33x45-T3"]
    inp = R.inputs(c)
    got = R.as_got(R.reference(c, inp))
    ref = R.reference(c, inp)
    far = np.argmax(np.abs(R.mc_uncertainty(inp["mc"], c.T).v - inp["thr"]))
    got["mask"].reshape(-1)[far] ^= 1
    assert any(b.startswith("mask") for b in R.compare(ref, got)[1])
    got["mask"].reshape(-1)[far] = 255                               # a byte that is neither 0 nor 1
    assert any(b.startswith("mask") for b in R.compare(R.reference(c, inp), got)[1])


def test_a_value_that_is_not_a_number_is_rejected():
    c = R.BY_ID["pair-randn2"]
    inp = R.inputs(c)
    ref = R.reference(c, inp)
    got = R.as_got(ref)
    got["kl_map"][0, 0, 0] = np.nan
    assert R.compare(ref, got)[1]
    c = R.BY_ID["pairp-01"]
    inp = R.inputs(c)
    ref = R.reference(c, inp)
    got = R.as_got(ref)
    i = tuple(np.argwhere(ref.nonfinite == 1)[0])
    got["kl_map"][i] = np.nan                                        # +inf expected, NaN returned: another kind
    assert R.compare(ref, got)[1]


# ---- the table ----------------------------------------------------------------------------------------------------------------
def test_case_table_is_consistent():
    assert len(R.BY_ID) == len(R.CASES)
    by = lambda *e: [c for c in R.CASES if c.entry in e]
    C_all = set(R.CLASSES)
    for e in ("mc_fwd", "mc_bwd", "cct_fwd", "cct_bwd", "rot_fwd", "rot_bwd", "pair_fwd", "mse_bwd", "kl_bwd", "klmap_bwd", "entropy"):
        assert {c.shape[1] for c in by(e)} == C_all, e
    for mode in ("mt", "mask"):
        assert {c.shape[1] for c in by("mc_fwd") if c.mode == mode} == C_all and {c.shape[1] for c in by("mc_bwd") if c.mode == mode} == C_all
    um = [c for c in by("mc_fwd") if c.mode == "mask"]
    assert {(c.T, (c.shape[0],) + c.shape[2:]) for c in um} >= {(T, s) for T in (0, 1, 3, 16) for s in R.RAGGED}
    assert {c.unc for c in um} == {True, False} and {c.thr_q for c in um} >= {0.25, 0.5, 0.9}
    assert all(any((c.shape[0] * c.shape[2] * c.shape[3]) % 256 for c in um if c.T == T) for T in (0, 1, 3, 16))     # a partial last block
    for e in ("cct_fwd", "cct_bwd"):
        assert {(c.shape[1], R.cct_vec(c)) for c in by(e)} == {(C, v) for C in C_all for v in (False, True)}
        assert {c.D for c in by(e)} == {2, 3, 8} and any(c.b0 > 0 for c in by(e))
        forced = [c for c in by(e) if not R.cct_vec(c) and (c.shape[2] * c.shape[3]) % 4 == 0]
        assert {c.shape[1] for c in forced} == C_all and all(sum(o % 4 != 0 for o in c.offs) == 1 for c in forced)
        for c in by(e):                                  # the ids say which form runs
            tag = c.id.split("-")[-1]
            assert tag not in ("v1", "v4", "forced") or R.cct_vec(c) == (tag == "v4"), c.id
        ragged = [c for c in by(e) if (c.shape[2] * c.shape[3]) % 4 and c.b0 > 0 and (c.Btot or 0) > c.b0 + c.shape[0] - 1]
        assert {c.shape[1] for c in ragged} == C_all     # the one-pixel form on a ragged plane inside a window, for every C
        assert any(R.cct_vec(c) and c.shape[2:] == (1, 40) for c in by(e))
        assert any(R.cct_vec(c) and c.shape[0] * c.shape[2] * c.shape[3] // 4 > R.MAX_BLOCKS * R.THREADS for c in by(e))
        assert any(not R.cct_vec(c) and c.shape[0] * c.shape[2] * c.shape[3] > R.MAX_BLOCKS * R.THREADS for c in by(e))
    for e in ("mc_fwd", "mc_bwd", "pair_fwd", "mse_bwd", "kl_bwd", "klmap_bwd", "entropy"):
        assert any(c.shape[0] * c.shape[2] * c.shape[3] > R.MAX_BLOCKS * R.THREADS for c in by(e)), e
        assert {(c.shape[0],) + c.shape[2:] for c in by(e)} >= set(R.RAGGED), e
    for e in ("rot_fwd", "rot_bwd"):
        assert {c.k for c in by(e) if c.shape[2] != c.shape[3]} == {0, 1, 2, 3} and any(c.r_b0 != c.u_b0 and c.r_b0 > 0 for c in by(e))
        cap = [c for c in by(e) if -(-c.shape[2] // R.TILE) * -(-c.shape[3] // R.TILE) * c.shape[0] > R.MAX_BLOCKS]
        assert {c.k % 2 for c in cap} == {0, 1} and all(c.shape[3] % R.TILE for c in cap)
    r90 = by("rot90")
    assert {c.k for c in r90 if c.shape[2] != c.shape[3]} == {0, 1, 2, 3} and {c.k for c in r90 if not c.rot_out} == {0, 1, 2, 3}
    big = [c for c in r90 if int(np.prod(c.shape)) > 2 * R.MAX_BLOCKS * R.THREADS]
    assert any(all(o % 4 == 0 for o in c.offs) and np.prod(c.shape) % 4 == 0 for c in big) and any(np.prod(c.shape) % 4 for c in big)
    assert any(any(o % 4 for o in c.offs) and np.prod(c.shape) % 4 == 0 for c in big)
    assert any(c.hinted for c in r90) and any(c.amax for c in r90)
    for e in ("mc_fwd", "cct_fwd", "rot_fwd", "pair_fwd", "mse_bwd", "kl_bwd", "klmap_bwd", "mc_bwd", "cct_bwd", "rot_bwd"):
        assert {c.regime for c in by(e)} >= set(R.REGIMES), e
    assert {c.regime for c in by("pair_fwd") if c.probs} >= {"probs", "probs01"}
    assert {frozenset(c.outs) for c in by("pair_fwd") if not c.probs} == {frozenset(s) for s in (
        ("mse_map",), ("kl_map",), ("kl_mean",), ("mse_map", "kl_map"), ("mse_map", "kl_mean"), ("kl_map", "kl_mean"), ("mse_map", "kl_map", "kl_mean"))}
    assert {c.outs for c in by("klmap_bwd")} == {("da", "db"), ("da",), ("db",)}
    assert {c.outs for c in by("entropy")} == {("ent_map", "ent_mean"), ("ent_map",), ("ent_mean",)}
    assert {c.gnull for c in by("kl_bwd")} == {True, False}
    ema = by("ema")
    assert {len(c.numels) for c in ema} >= {1, 128, 129, 257} and set().union(*(set(c.numels) for c in ema)) >= set(R.EMA_SIZES)
    assert any(c.step == 0 for c in ema)
    sides = {(c.offe[i % len(c.offe)] % 4 != 0, c.offp[i % len(c.offp)] % 4 != 0) for c in ema for i in range(len(c.numels))}
    assert sides == {(False, False), (True, False), (False, True), (True, True)}
    nz = by("noise", "noise_apply")
    assert {c.T for c in nz} >= {0, 1, 3, 16}
    for e in ("noise", "noise_apply"):
        assert any((1 + c.T) * int(np.prod(c.shape)) > 4 * R.NOISE_BLOCKS * R.THREADS for c in by(e)), e
    assert any(int(np.prod(c.shape[1:])) % 4 for c in nz) and any(c.offset >> 31 for c in by("noise"))


def test_mask_mode_cases_have_a_mixed_mask():
    """Every masked case of more than one pixel keeps some pixels and drops some, so the masked sums and the gradient are compared
    on both kinds (all-equal Monte-Carlo logits apart: u = ln C on every pixel, the mask is whole)."""
    for c in (c for c in R.CASES if c.entry in ("mc_fwd", "mc_bwd") and c.mode == "mask"):
        inp = R.inputs(c)
        m = R.reference(c, inp).mask_ref if c.entry == "mc_fwd" else inp["mask"]
        if m.size == 1 or (c.entry == "mc_fwd" and c.regime == "equal"):
            assert m.all(), c.id
        else:
            assert 0 < m.mean() < 1, (c.id, m.mean())


def _built():
    from uaps_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libuaps_hip.so is not built")
    return norm_act_kernel_symbols(_lib.LIB_PATH, kernel_pattern(R.KERNEL_NAMES))


def test_cases_cover_every_kernel_and_name_none_that_does_not_exist():
    built = _built()
    assert len(built) == 105, sorted(built)
    named = set().union(*(c.kernels for c in R.CASES))
    assert named == built, ("no case reaches", sorted(built - named), "no such kernel", sorted(named - built))


def test_every_kernel_of_the_three_sources_is_in_the_filter():
    """The name filter lists every __global__ of loss_mean_teacher.hip and loss_cct_dct.hip, and of pair_ops.hip all but its joins
    (tests/ops_ref.py has those)."""
    import re
    GLOBAL = r"__global__(?:\s+__launch_bounds__\([^)]*\))?\s+void\s+(\w+)\s*\("
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uaps_amd", "csrc")
    found = set()
    for f in ("loss_mean_teacher.hip", "loss_cct_dct.hip", "pair_ops.hip"):
        found |= set(re.findall(GLOBAL, open(os.path.join(src, f)).read()))
    assert found - {"add_relu_kernel", "relu_bwd_kernel", "relu_bwd_sum_kernel", "cat2_amax_kernel"} == set(R.KERNEL_NAMES)


def test_grid_rule_matches_the_launchers():
    assert R.grid_for(0) == 1 and R.grid_for(256) == 1 and R.grid_for(257) == 2 and R.grid_for(263153) == 1024 and R.grid_for(262144) == 1024
    assert R.grid_for(262144 - 256) == 1023 and R.grid_for(17 * 270000 // 4, R.NOISE_BLOCKS) == 4096
