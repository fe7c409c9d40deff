"""The references of tests/ops_ref.py on the CPU: the host Philox and u01 against known answers, every reference against torch in float64
(F.interpolate(align_corners=True) and its autograd, max_pool2d, torch.optim.Adam, a restatement of the reference model's
FeatureDropout), the comparison code of tests/test_gpu_ops_forms.py passing the unmutated restatements and rejecting every mutant, and
the case table naming exactly the kernels of perturb.hip, resample.hip, adam.hip and the joins of pair_ops.hip that the built code
object holds."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ops_ref as R
from bn_ref import keep_mask, philox4x32_10
from test_bn_ref import kernel_pattern, norm_act_kernel_symbols

F32 = np.float32


# ---- Philox, u01 ----------------------------------------------------------------------------------------------------------------
def test_words_are_philox_with_the_uaps_counter_layout():
    """words(seed, ctr) = Philox4x32-10 of (ctr low, ctr high, "UAPS", 0) under (seed low, seed high); Random123's known answer."""
    assert tuple(int(v) for v in philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    seed, ctr = 0xFEDCBA9876543210, np.array([0, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3], np.uint64)
    w = R.words(seed, ctr)
    for i, c in enumerate(ctr):
        want = philox4x32_10(int(c) & 0xFFFFFFFF, int(c) >> 32, 0x55415053, 0, seed & 0xFFFFFFFF, seed >> 32)
        assert tuple(int(v) for v in w[i]) == tuple(int(v) for v in want)
    assert not np.array_equal(R.words(seed, ctr, "no_hi")[3], w[3]) and np.array_equal(R.words(seed, ctr, "no_hi")[1], w[1])


def test_u01_known_answers():
    u = R.u01(np.array([0, 0xFF, 0x100, 0x80000000, 0xFFFFFFFF], np.uint32))
    assert u.dtype == F32 and list(u) == [0.0, 0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24]


def test_element_draws_match_the_dropout_mask_of_bn_ref():
    n, seed, off = 37, 0x0123456789ABCDEF, 2 ** 32 - 3
    assert np.array_equal(R.element_u01(seed, off, n) >= F32(0.4), keep_mask(n, 0.4, seed, off))
    assert np.array_equal(R.element_u01(seed, off, n, "ctr_shift") >= F32(0.4), keep_mask(n, 0.4, seed, off, ctr_shift=1))


def test_noise_draw_is_exact_in_float32():
    """(2 u01 - 1) range: 2 u01 - 1 is representable, so the float32 result is the float64 product rounded once."""
    u = R.element_u01(7, 0, 4096).astype(np.float64)
    assert np.array_equal(R.noise_of(7, 0, 4096, 0.3), ((2 * u - 1) * float(F32(0.3))).astype(F32))


# ---- the references against torch float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 2), (2, 3), (5, 6), (9, 33), (33, 18)])
def test_up2x_matches_torch_interpolate_and_its_autograd(h, w):
    rng = np.random.default_rng(h * 100 + w)
    low = rng.standard_normal((2, 3, h, w)).astype(F32)
    t = torch.from_numpy(low.astype(np.float64)).requires_grad_(True)
    up = F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)
    val, bar = R.up2x(low)
    # torch forms the source index in float64 here, the reference in float32 as the kernel does: the weights differ by ~2^-24 n
    tol = 2.0 ** -22 * max(h, w) * np.abs(low).max()
    assert np.abs(val - up.detach().numpy()).max() <= tol
    assert np.all(bar >= 0) and bar.shape == val.shape
    dout = rng.standard_normal(up.shape)
    up.backward(torch.from_numpy(dout))
    adj, abar = R.up2x_adjoint(dout.astype(F32))
    assert np.abs(adj - t.grad.numpy()).max() <= 2.0 ** -21 * max(h, w) * np.abs(dout).max() * 4
    # the adjoint identity holds exactly for the reference's own weights: <up(x), d> = <x, adj(d)>
    d32 = dout.astype(F32).astype(np.float64)
    assert abs((val * d32).sum() - (low * adj).sum()) <= 1e-9 * np.abs(val * d32).sum()


def test_taps_follow_aten():
    i0, i1, l0, l1 = R.taps(5)
    r = F32(4) / F32(9)
    assert i0.tolist() == [int(F32(r * F32(o))) for o in range(10)] and i1[-1] == 4 and i0[-1] == 4 and l1[-1] == 0
    assert np.all(l0 + l1 == 1) or np.abs(l0 + l1 - 1).max() <= 2.0 ** -23


@pytest.mark.parametrize("special", [False, True])
def test_maxpool_matches_torch(special):
    x = R.pool_special() if special else np.random.default_rng(3).standard_normal((3, 5, 6, 24)).astype(F32)
    W = x.shape[-1]
    out, idx = R.maxpool2x2(x)
    to, ti = F.max_pool2d(torch.from_numpy(x), 2, return_indices=True)
    assert R.bits_differ(out, to.numpy()) == 0
    assert np.array_equal(idx, ((ti // W) % 2 * 2 + (ti % W) % 2).to(torch.uint8).numpy())
    if special:
        assert np.isnan(out).sum() == 10 and (out == -np.inf).sum() == 1 and {0, 1, 2, 3} <= set(idx.reshape(-1).tolist())
        g = np.arange(out.size, dtype=F32).reshape(out.shape) + 1
        assert (R.unpool(g, idx) != 0).sum() == out.size


@pytest.mark.parametrize("wd,step", [(0.0, 1), (0.01, 1000)])
def test_adam_matches_torch_optim(wd, step):
    c = R.Case(f"torch-adam-{wd}-{step}", "adam", numels=(257,), wd=wd, step=step)
    t = R.inputs(c)["t"][0]
    p = torch.nn.Parameter(torch.from_numpy(t["p"].astype(np.float64)))
    p.grad = torch.from_numpy(t["g"].astype(np.float64))
    opt = torch.optim.Adam([p], weight_decay=wd, **{k: v for k, v in zip(("lr", "betas", "eps"), (1e-3, (0.9, 0.999), 1e-8))})
    opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(t["m"].astype(np.float64)),
                        exp_avg_sq=torch.from_numpy(t["v"].astype(np.float64)))
    opt.step()
    ref = R.adam(t["p"], t["g"], t["m"], t["v"], wd=wd, step=step, **R.ADAM_HYPER)
    np.testing.assert_allclose(ref["p"], p.detach().numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(ref["m"], opt.state[p]["exp_avg"].numpy(), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(ref["v"], opt.state[p]["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-24)


def test_feature_dropout_matches_the_model():
    """utilities/UAPS_unet.py's FeatureDropout restated: attention = mean over channels, threshold = max over pixels * u,
    mask = attention < threshold, x * mask.  In float64 on float32-exact data the strict comparison is the float32 one wherever the
    float32 attention is exact (every channel equal and C a power of two: the tie case) and everywhere else but at roundings."""
    c = R.BY_ID["fdrop-tie"]
    inp = R.inputs(c)
    x = torch.from_numpy(inp["x"].astype(np.float64))
    att = torch.mean(x, dim=1, keepdim=True)
    mx, _ = torch.max(att.view(x.size(0), -1), dim=1, keepdim=True)
    thr = (mx * float(F32(c.u))).view(x.size(0), 1, 1, 1).expand_as(att)
    want = x.mul((att < thr).float())
    ref = R.reference(c, inp)
    assert np.array_equal(ref.exact["y"].astype(np.float64), want.numpy())
    keep = ref.exact["keep"].reshape(2, 4, 8)
    assert keep[0, 1, 1] == 0 and keep[0, 2, 2] == 1 and keep[0, 0, 0] == 0          # at the threshold: dropped; one ulp below: kept
    # random data: the float32 attention is within C 2^-24 mean|x| of the model's, and away from the threshold the masks agree
    c = R.BY_ID["fdrop-c20"]
    inp = R.inputs(c)
    x = torch.from_numpy(inp["x"].astype(np.float64))
    att = x.mean(1).view(2, -1).numpy()
    ref = R.reference(c, inp)
    assert np.abs(ref.exact["att"] - att).max() <= 20 * R.EPS24 * np.abs(inp["x"]).mean(1).max()
    thr = att.max(1, keepdims=True) * float(F32(c.u))
    clear = np.abs(att - thr) > 1e-5
    assert np.array_equal((att < thr)[clear], ref.exact["keep"].astype(bool)[clear])


def test_feature_dropout_edges():
    for cid, kept in (("fdrop-negative", 1), ("fdrop-zero", 0)):
        c = R.BY_ID[cid]
        ref = R.reference(c, R.inputs(c))
        assert np.all(ref.exact["keep"] == kept), cid
    assert list(R.att_max(np.array([[-0.0, 0.0], [-2.0, -1.0], [0.0, -0.0]], F32)).view(np.uint32)) == [0, 0xBF800000, 0]


def test_attention_orders_differ_and_both_hold_the_float64_mean():
    c = R.BY_ID["stats-split-68"]
    inp = R.inputs(c)
    a, b = R.attention(inp["x"], True), R.attention(inp["x"], False)
    assert R.bits_differ(a, b) > 0
    x64 = inp["x"].astype(np.float64).reshape(1, 68, -1)
    for att in (a, b):
        assert R.bar_ratio(att, x64.mean(1), 68 * R.EPS24 * np.abs(x64).mean(1)) <= 1


def test_device_drawn_threshold_does_not_depend_on_the_contraction():
    """0.7f + 0.2f u01: fused or not, the masks of every case that lets the kernel draw u are the same."""
    n = 0
    for c in R.CASES:
        if c.entry == "fanout" and any(v < 0 for v in c.u) and 3 in c.modes:
            inp = R.inputs(c)
            a, b = R.reference(c, inp), R.reference(c, inp, mut="unfused")
            assert all(R.bits_differ(a.exact[k], b.exact[k]) == 0 for k in a.exact), c.id
            n += 1
    assert n >= 2


def test_confusion_and_joins_against_torch():
    c = R.BY_ID["conf-c4"]
    inp = R.inputs(c)
    z, y = torch.from_numpy(inp["z"]), torch.from_numpy(inp["y"])
    want = np.zeros((4, 4), np.int64)
    arg = np.zeros(y.shape, np.int64)
    for k in range(1, 4):                      # the lowest index wins a tie: a later class must be strictly larger
        arg = np.where(inp["z"][:, k] > np.take_along_axis(inp["z"], arg[:, None], 1)[:, 0], k, arg)
    ok = (inp["y"] >= 0) & (inp["y"] < 4)
    np.add.at(want, (inp["y"][ok], arg[ok]), 1)
    assert np.array_equal(R.confusion(inp["z"], inp["y"]), want) and want.sum() == ok.sum() < y.numel()
    assert (inp["z"].max(1, keepdims=True) == inp["z"]).sum(1).max() >= 2          # the table's data does hold ties
    c = R.BY_ID["add_relu-special"]
    inp = R.inputs(c)
    a, b = torch.from_numpy(inp["a"]), torch.from_numpy(inp["b"])
    out = R.add_relu(inp["a"], inp["b"])
    want = torch.relu(a + b).numpy()
    want = np.where(want == 0, F32(0), want)          # torch.relu keeps a -0.0 sum; the join writes +0.0 (include/uaps_hip.h)
    assert R.bits_differ(out, want) == 0 and np.isnan(out).any() and np.isinf(out).any() and (out == 0).any()
    assert not np.signbit(out[~np.isnan(out)]).any()
    assert R.amax_after(0.5, out, False) == float(np.nanmax(out)) == np.inf
    o = torch.from_numpy(inp["b"])
    assert R.bits_differ(R.relu_bwd([inp["a"]], inp["b"]), torch.where(o > 0, a, torch.zeros_like(a)).numpy()) == 0


# ---- the comparisons of the GPU test: correct results pass, mutants do not ----------------------------------------------------
SMALL = [c.id for c in R.CASES if c.id not in ("fdrop-grid-cap", "noise-two-trips", "conf-loop", "adam-grid-cap", "adam-grid-cap-misaligned")]


@pytest.mark.parametrize("cid", SMALL)
def test_unmutated_reference_passes_its_own_comparison(cid):
    c = R.BY_ID[cid]
    inp = R.inputs(c)
    ref = R.reference(c, inp)
    got = R.as_got(ref)
    if c.entry == "adam":                      # the kernel's operation order in float32
        sc = R.adam_scalars(R.ADAM_HYPER["lr"], R.ADAM_HYPER["b1"], R.ADAM_HYPER["b2"], 7) if c.state else None
        got["adam"] = [{k: R.adam(t["p"], t["g"], t["m"], t["v"], wd=c.wd, step=c.step, scalars=sc, dtype=np.float32, **R.ADAM_HYPER)[k]
                        for k in ("p", "m", "v")} for t in inp["t"]]
    ratios, bad = R.compare(ref, got)
    assert not bad, bad
    assert ref.exact or ref.f64 or ref.adam


MUTANTS = [
    ("ctr_shift", "noise-vec"), ("ctr_shift", "bern-n7"), ("ctr_shift", "fanout-pow2"), ("ctr_shift", "fanin-pow2"),
    ("word_rot", "noise-size"), ("word_rot", "bern-n4101"), ("word_rot", "fanout-neither"), ("word_rot", "fanin-neither"),
    ("no_hi", "noise-carry"), ("no_hi", "noise-carry-scalar"), ("no_hi", "bern-n7"), ("no_hi", "fanout-g4"), ("no_hi", "fanin-n8"),
    ("gt", "bern-tie"), ("le", "fdrop-tie"),
    ("other_order", "stats-split-2x2"), ("other_order", "stats-split-68"), ("other_order", "stats-split-hw4096"),
    ("other_order", "stats-plain-hw4100"), ("other_order", "stats-scalar-offx"),
    ("wrong_group", "fanout-pow2"), ("wrong_group", "fanout-n8"), ("wrong_group", "fanin-pow2"), ("wrong_group", "fanin-g4"),
    ("drop_term", "fanin-pow2"), ("drop_term", "fanin-n8"), ("drop_term", "fanin-neither"),
    ("last_wins", "pool-special"), ("last_wins", "conf-c4"),
    ("half_pixel", "up-tiled-5x16"), ("half_pixel", "up-cat-2x2"), ("half_pixel", "up-scalar-w3"), ("half_pixel", "upb-5x6"),
    ("half_pixel", "upb-32x32"),
    ("no_clamp", "up-clamp-cat"), ("no_clamp", "up-clamp-scalar"),
    ("eps_inside", "adam-tiny"), ("no_bias_correction", "adam-1"), ("no_bias_correction", "adam-48"), ("decoupled_wd", "adam-48"),
    ("nan_to_zero", "add_relu-special")]


@pytest.mark.parametrize("mut,cid", MUTANTS)
def test_comparison_rejects_mutant(mut, cid):
    c = R.BY_ID[cid]
    inp = R.inputs(c)
    ratios, bad = R.compare(R.reference(c, inp), R.as_got(R.reference(c, inp, mut=mut)))
    assert bad, (mut, cid, ratios)


def test_every_listed_mutant_is_tried():
    assert {m for m, _ in MUTANTS} == {"ctr_shift", "word_rot", "no_hi", "gt", "le", "other_order", "wrong_group", "drop_term", "last_wins",
                                       "half_pixel", "no_clamp", "eps_inside", "no_bias_correction", "decoupled_wd", "nan_to_zero"}


def test_a_missing_clamp_changes_no_finite_result():
    """Why the clamp cases carry an inf: the last output of every size lands exactly on the last input, the second tap has weight 0."""
    for n in range(1, 130):
        i0, i1, l0, l1 = R.taps(n)
        assert i0[-1] == n - 1 and l1[-1] == 0 and i1.max() == n - 1


# ---- the table ----------------------------------------------------------------------------------------------------------------
def test_case_table_is_consistent():
    assert len(R.BY_ID) == len(R.CASES)
    by = lambda e: [c for c in R.CASES if c.entry == e]
    assert {c.shape for c in by("noise")} >= {(3, 2, 2, 4), (2, 3, 3, 3), (1, 33, 256, 256)}
    assert any(c.offset == 2 ** 32 - 3 for c in by("noise")) and any(c.seed >> 32 and c.seed & 0xFFFFFFFF for c in by("noise"))
    assert 33 * 256 * 256 // 4 > R.MAX_BLOCKS * R.THREADS
    assert {c.n for c in by("bernoulli")} >= {1, 3, 4, 7, 4101} and {c.p for c in by("bernoulli")} >= {0.0, 0.999}
    assert {c.shape[1] for c in by("fdrop")} >= {1, 3, 16, 20, 35} and (2048, 1, 64, 64) in {c.shape for c in by("fdrop")}
    assert {c.special for c in by("fdrop")} >= {"tie", "neg", "zero"}
    assert {c.shape for c in by("fdrop_stats")} >= {(2, 64, 2, 2), (1, 68, 4, 72), (1, 64, 64, 64), (1, 64, 41, 100)}
    fo = by("fanout")
    assert {c.shape for c in fo} >= {(4, 16, 8, 8), (2, 3, 8, 8), (2, 5, 6, 6)} and {c.groups for c in fo} == {1, 2, 3, 4}
    assert {len(c.modes) for c in fo} >= {1, 8} and any(c.state for c in fo) and any(min(c.u) < 0 for c in fo)
    for k in range(3):                          # modes 1, 2, 3 in every one of the first three positions
        assert {c.modes[k] for c in fo if len(c.modes) > k} >= {1, 2, 3}
    fi = by("fanin")
    assert set().union(*(set(c.modes) for c in fi)) == {0, 1, 2, 3, 4} and {c.shape[3] for c in fi if 4 in c.modes} >= {8, 12}
    for c in fo + fi:
        B, C, H, W = c.shape
        assert B % c.groups == 0 and (H * W) % 4 == 0 and (4 not in c.modes or (H % 2 == 0 and W % 4 == 0)), c.id
        assert B * C * H * W // 4 < 2 ** 32          # the 64-bit division of fan_divmod stays out of reach (2^32 float4 = 64 GiB)
    assert {c.count for c in by("sum")} >= {1, 3, 4, 5, 1027} and {c.n for c in by("sum")} == {1, 2, 3, 4}
    assert {c.shape[1] for c in by("confusion")} >= {1, 4, R.MAX_CLASSES} and any(np.prod(c.shape) // c.shape[1] > 512 * 256 for c in by("confusion"))
    assert {(c.h, c.w) for c in by("up_fwd") if c.Cs == 0 and not c.offo} >= {(1, 2), (5, 16), (33, 18), (3, 32), (9, 34), (32, 32), (35, 34)}
    assert {(c.h, c.w) for c in by("up_bwd")} >= {(1, 1), (5, 6), (9, 33), (2, 3), (32, 32), (33, 34), (40, 36)}
    assert any(c.offd % 4 and (2 * c.w) % 4 == 0 for c in by("up_bwd"))
    for e in ("add_relu", "relu_bwd", "cat2", "relu_bwd_sum"):
        assert {c.n for c in by(e)} >= {1, 3, 4, 5, 1031} and any(c.special for c in by(e)), e
    assert {c.k for c in by("relu_bwd_sum")} == {1, 2, 3, 4}
    assert {len(c.numels) for c in by("adam")} >= {1, 48, 49, 97} and {c.wd for c in by("adam")} == {0.0, 0.01}
    assert {c.step for c in by("adam")} >= {1, 1000} and any(262144 * 4 + 7 in c.numels for c in by("adam"))


def _built():
    from uaps_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libuaps_hip.so is not built")
    return norm_act_kernel_symbols(_lib.LIB_PATH, kernel_pattern(R.KERNEL_NAMES))


def test_cases_cover_every_kernel_and_name_none_that_does_not_exist():
    built = _built()
    assert len(built) == 34, sorted(built)
    named = set().union(*(c.kernels for c in R.CASES))
    assert named == built, ("no case reaches", sorted(built - named), "no such kernel", sorted(named - built))


def test_every_kernel_of_the_four_sources_is_in_the_filter():
    """The name filter lists every __global__ of perturb.hip, resample.hip and adam.hip, and the four joins of pair_ops.hip."""
    import re
    GLOBAL = r"__global__(?:\s+__launch_bounds__\([^)]*\))?\s+void\s+(\w+)\s*\("
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uaps_amd", "csrc")
    found = set()
    for f in ("perturb.hip", "resample.hip", "adam.hip"):
        found |= set(re.findall(GLOBAL, open(os.path.join(src, f)).read()))
    assert found | {"add_relu_kernel", "relu_bwd_kernel", "relu_bwd_sum_kernel", "cat2_amax_kernel"} == set(R.KERNEL_NAMES)
    joins = set(re.findall(GLOBAL, open(os.path.join(src, "pair_ops.hip")).read()))
    assert {"add_relu_kernel", "relu_bwd_kernel", "relu_bwd_sum_kernel", "cat2_amax_kernel"} <= joins


def test_removing_a_case_uncovers_its_kernel():
    """The cases that alone reach a kernel: without any one of them the coverage test names that kernel."""
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
