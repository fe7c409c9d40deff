"""UCC on the GPU: the kernels of csrc/loss_ucc.hip against the reference-generated fixture g10_ucc.npz (and g8_sibling.npz), against a
torch `where` restatement of the cut-mix and a float64 restatement of UCC/UCC_train.py:186-246 built from oracle.uaps_oracle;
UNet_UAPS.forward_groups; whole trainer steps against a float64 oracle; checkpoints, the epoch loop and the kernels one step launches."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "g10_ucc.npz")
GOLD8 = os.path.join(HERE, "golden", "g8_sibling.npz")


# ---- restatements -------------------------------------------------------------------------------------------------------------------------

def _inside(r, H, W, device="cpu"):
    yy = torch.arange(H, device=device).view(H, 1)
    xx = torch.arange(W, device=device).view(1, W)
    return (yy >= int(r[1])) & (yy < int(r[2])) & (xx >= int(r[3])) & (xx < int(r[4])) & bool(r[0])


def _cutmix_where(x_l, y_l, x_wk, x_st, rl, ru):
    """cross_cutmix.py:78-123 as torch.where over the rectangles: (mixed [3B,...], mixed labels)."""
    B, _, H, W = x_l.shape
    out_l, out_y, out_wk, out_st = [], [], [], []
    for i in range(B):
        m1, m2 = _inside(rl[i], H, W, x_l.device), _inside(ru[i], H, W, x_l.device)
        out_l.append(torch.where(m1, x_l[(i + 1) % B], x_l[i]))
        out_y.append(torch.where(m1, y_l[(i + 1) % B], y_l[i]))
        out_wk.append(torch.where(m2, out_l[i], x_wk[i]))
        out_st.append(torch.where(m2, out_l[i], x_st[i]))
    return torch.stack(out_l + out_wk + out_st), torch.stack(out_y)


def _ucc64(z1, z2, y, B, p1, p2):
    """UCC_train.py:186-240 on logits of any float dtype with GIVEN pseudo-labels p1, p2 [B,H,W] (int64).  Returns a dict: ce[4],
    dice[4] in the term order of uaps_amd.ucc.TERMS, sup, ps_1, ps_2, ps and the variance maps v1, v2."""
    from oracle import uaps_oracle as O

    def pair(z, t):
        return O.cross_entropy(z, t), O.dice_loss(t.unsqueeze(1), z)

    def variance(a, b):                                       # sum_c KLDivLoss(none)(log_softmax(a), softmax(b))
        return (torch.softmax(b, dim=1) * (torch.log_softmax(b, dim=1) - torch.log_softmax(a, dim=1))).sum(dim=1)
    l1, l2, wk1, wk2, st1, st2 = z1[:B], z2[:B], z1[B:2 * B], z2[B:2 * B], z1[2 * B:], z2[2 * B:]
    terms = [pair(l1, y), pair(l2, y), pair(st1, p1), pair(st2, p2)]
    sup = 0.5 * (terms[0][0] + terms[0][1]) + 0.5 * (terms[1][0] + terms[1][1])
    v1, v2 = variance(wk1, st2), variance(st1, wk2)
    ps_1 = torch.mean(0.5 * (terms[2][0] + terms[2][1]) * torch.exp(-v1)) + torch.mean(v1)
    ps_2 = torch.mean(0.5 * (terms[3][0] + terms[3][1]) * torch.exp(-v2)) + torch.mean(v2)
    return {"ce": [t[0] for t in terms], "dice": [t[1] for t in terms], "sup": sup, "ps_1": ps_1, "ps_2": ps_2, "ps": ps_1 + ps_2,
            "v1": v1, "v2": v2}


def _argmax_first(z):
    """arg-max over the classes of fp32 logits, the lowest index among equal values (numpy's argmax returns the first)."""
    return torch.from_numpy(np.argmax(z.detach().cpu().numpy(), axis=1).astype(np.int64))


# ---- 1. cut-mix ----------------------------------------------------------------------------------------------------------------------------

def test_cutmix_batch_is_bit_equal_to_the_reference_fixture():
    import random
    from uaps_amd import ucc
    g = np.load(GOLD)
    seed = int(g["mix_seed"])
    B, _, H, W = g["mix_x_l"].shape
    np_rng, py_rng = np.random.RandomState(seed), random.Random(seed)
    rl = ucc.cutmix_rects(B, H, W, np_rng, py_rng, ucc.P_MIX)
    ru = ucc.cutmix_rects(B, H, W, np_rng, py_rng, ucc.P_CROSSMIX)
    t = {k: torch.tensor(g[k], device=DEV) for k in ("mix_x_l", "mix_y_l", "mix_x_wk", "mix_x_st")}
    out, y_out = ucc.cutmix_batch(t["mix_x_l"], t["mix_y_l"], t["mix_x_wk"], t["mix_x_st"], rl, ru)
    assert out.shape == (3 * B,) + g["mix_x_l"].shape[1:] and y_out.dtype == torch.int64
    got = out.cpu().numpy()
    assert np.array_equal(got[:B], g["mix_out_l"]) and np.array_equal(got[B:2 * B], g["mix_out_wk"])
    assert np.array_equal(got[2 * B:], g["mix_out_st"]) and np.array_equal(y_out.cpu().numpy(), g["mix_out_y"])


def _rect_cases(B, H, W):
    full, empty = (1, 0, H, 0, W), (1, H // 2, H // 2, 0, W)
    some = [(1, 0, max(1, H // 2), 0, max(1, W - 1)), (1, H // 3, H, W // 4, W), (1, 0, H, 0, W)]
    off = [(0,) + r[1:] for r in some]
    pick = lambda rows: np.array([rows[i % len(rows)] for i in range(B)], dtype=np.int32)
    return {"all_off": (pick(off), pick(off)), "all_on": (pick(some), pick(some[::-1])), "every_border": (pick([full]), pick([full])),
            "empty": (pick([empty]), pick([empty, some[0]])), "mixed": (pick([some[1], off[0]]), pick([off[1], some[0], some[1]]))}


@pytest.mark.parametrize("case", ["all_off", "all_on", "every_border", "empty", "mixed"])
@pytest.mark.parametrize("shape", [(1, 1, 2, 4), (3, 3, 37, 53), (2, 3, 16, 24)])
def test_cutmix_batch_is_bit_equal_to_torch_where(shape, case):
    """B = 1 pastes an image onto itself; (37, 53): the one-pixel-a-lane path; the others: four pixels a lane (H W % 4 == 0)."""
    from uaps_amd import bounds, ucc
    B, Ci, H, W = shape
    gen = torch.Generator().manual_seed(B * 7 + H)
    x_l, x_wk, x_st = (torch.randn(B, Ci, H, W, generator=gen).to(DEV) for _ in range(3))
    x_l[0, 0, 0, 0] = -0.0
    y_l = torch.randint(0, 4, (B, H, W), generator=gen).to(DEV)
    rl, ru = _rect_cases(B, H, W)[case]
    out, y_out = ucc.cutmix_batch(x_l, y_l, x_wk, x_st, rl, ru)
    ref, y_ref = _cutmix_where(x_l, y_l, x_wk, x_st, rl, ru)
    assert torch.equal(out, ref) and torch.equal(y_out, y_ref)
    if case == "all_off":
        assert torch.equal(out, torch.cat([x_l, x_wk, x_st])) and torch.equal(y_out, y_l)
    if case == "every_border":
        assert torch.equal(out[:B], torch.roll(x_l, -1, 0)) and torch.equal(out[B:2 * B], out[:B]) and torch.equal(out[2 * B:], out[:B])
    b = bounds.get(out)
    if b is not None:
        assert float(b[0].max()) == float(out.abs().max())


def test_cutmix_batch_amax_through_the_raw_entry_point():
    from uaps_amd import _lib, bounds
    B, Ci, H, W = 2, 3, 16, 24
    x_l, x_wk, x_st = torch.randn(B, Ci, H, W, device=DEV), torch.randn(B, Ci, H, W, device=DEV) * 3, torch.randn(B, Ci, H, W, device=DEV) * 5
    y_l = torch.zeros(B, H, W, dtype=torch.int64, device=DEV)
    rl, ru = _rect_cases(B, H, W)["mixed"]
    out, y_out = torch.empty(3 * B, Ci, H, W, device=DEV), torch.empty_like(y_l)
    am = bounds.new_amax(torch.device(DEV))
    rc = _lib.lib().uaps_ucc_cutmix_batch_h(_lib.mk_hints((), am), x_l.data_ptr(), x_wk.data_ptr(), x_st.data_ptr(), y_l.data_ptr(),
                                            rl.ctypes.data, ru.ctypes.data, B, Ci, H, W, out.data_ptr(), y_out.data_ptr(),
                                            _lib.current_stream(torch.device(DEV)))
    assert rc == 0
    assert torch.equal(out, _cutmix_where(x_l, y_l, x_wk, x_st, rl, ru)[0])
    assert float(am.max()) == float(out.abs().max())


# ---- 2. the loss kernels against the reference's fixtures ------------------------------------------------------------------------------------

def test_ucc_loss_matches_the_reference_fixture():
    """Tolerances of test_cps_loss_matches_the_reference_fixture (terms rtol 2e-5, gradients rtol 1e-3 / atol 2e-5 max|g|);
    pseudo-labels identical wherever the reference's top-2 softmax gap exceeds 1e-5, fewer than 1e-4 of the pixels different."""
    from uaps_amd import ucc
    g = np.load(GOLD)
    cw = float(g["cw"])
    z1 = torch.tensor(g["z1"], device=DEV, requires_grad=True)
    z2 = torch.tensor(g["z2"], device=DEV, requires_grad=True)
    y = torch.tensor(g["labels"], device=DEV)
    B = y.shape[0]
    sup, ps, scalars, p1, p2, v1, v2 = ucc.ucc_loss(z1, z2, y, B, return_var=True)
    (sup + cw * ps).backward()
    sc = ucc.ucc_scalars(scalars, z1.shape[1])
    print("ce", sc["ce"].tolist(), "dice", sc["dice"].tolist(), "sup", float(sup), "ps", float(ps), float(sc["ps_1"]), float(sc["ps_2"]))
    np.testing.assert_allclose(sc["ce"].cpu().double().numpy(), g["ce"], rtol=2e-5)
    np.testing.assert_allclose(sc["dice"].cpu().double().numpy(), g["dice"], rtol=2e-5)
    for got, key in ((sup, "sup"), (ps, "ps"), (sc["ps_1"], "ps_1"), (sc["ps_2"], "ps_2")):
        np.testing.assert_allclose(float(got), float(g[key]), rtol=2e-5, err_msg=key)
    np.testing.assert_allclose(float(sc["v1"]), float(g["variance_1"].mean(dtype=np.float64)), rtol=2e-5)
    np.testing.assert_allclose(float(sc["v2"]), float(g["variance_2"].mean(dtype=np.float64)), rtol=2e-5)
    assert float(sc["bad"]) == 0.0
    for got, key in ((v1, "variance_1"), (v2, "variance_2")):
        np.testing.assert_allclose(got.cpu().numpy(), g[key], rtol=1e-3, atol=2e-5 * np.abs(g[key]).max(), err_msg=key)
    for got, key in ((z1.grad, "dz1"), (z2.grad, "dz2")):
        ref = g[key]
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-3, atol=2e-5 * np.abs(ref).max(), err_msg=key)
    differ = 0
    for got, key, gap in ((p1, "pseudo1", "gap1"), (p2, "pseudo2", "gap2")):
        assert got.dtype == torch.uint8 and tuple(got.shape) == g[key].shape
        ne = got.cpu().numpy() != g[key]
        assert not (ne & (g[gap] > 1e-5)).any(), key
        differ += int(ne.sum())
    assert differ < 1e-4 * 2 * g["pseudo1"].size


@pytest.mark.parametrize("C", [4, 2])
def test_ucc_loss_on_the_sibling_fixture_embedded_beside_labelled_rows(C):
    """g8's UCC logits as rows [B:3B] beside arbitrary labelled rows: ps, ps_1, ps_2 and the four gradient blocks at the tolerances
    tests use for g8 (values rtol 2e-5; gradients rtol 1e-3 / atol 2e-5 max|g|)."""
    from uaps_amd import ucc
    g = np.load(GOLD8)
    wk1, wk2, st1, st2 = (torch.tensor(g[f"ucc{C}_{k}"]) for k in ("u1wk", "u2wk", "u1st", "u2st"))
    B, _, H, W = wk1.shape
    gen = torch.Generator().manual_seed(C)
    lab1, lab2 = torch.randn(B, C, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen)
    y = torch.randint(0, C, (B, H, W), generator=gen).to(DEV)
    z1 = torch.cat([lab1, wk1, st1]).to(DEV).requires_grad_(True)
    z2 = torch.cat([lab2, wk2, st2]).to(DEV).requires_grad_(True)
    sup, ps, scalars, _, _ = ucc.ucc_loss(z1, z2, y, B)
    ps.backward()
    sc = ucc.ucc_scalars(scalars, C)
    for got, key in ((ps, "ps_loss"), (sc["ps_1"], "ps_1_wk"), (sc["ps_2"], "ps_2_st")):
        np.testing.assert_allclose(float(got), float(g[f"ucc{C}_{key}"]), rtol=2e-5, err_msg=key)
    for got, key in ((z1.grad[B:2 * B], "du1wk"), (z2.grad[B:2 * B], "du2wk"), (z1.grad[2 * B:], "du1st"), (z2.grad[2 * B:], "du2st")):
        ref = g[f"ucc{C}_{key}"]
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-3, atol=2e-5 * np.abs(ref).max(), err_msg=key)
    assert float(z1.grad[:B].abs().max()) == 0.0 and float(z2.grad[:B].abs().max()) == 0.0      # ps does not reach the labelled rows


# ---- 3. float64 sweep -----------------------------------------------------------------------------------------------------------------------

_SWEEP = [(B, C, H, W) for C in (2, 4, 7, 8) for H, W in ((37, 53), (1, 40), (16, 24)) for B in (1, 2, 3)] + [(16, 4, 256, 256)]
# Bars: 1e-5 (the CPS sweep's) on the terms, the variance maps (of max v), the gradients and the class sums of a pixel's gradient (of
# max|g|).  A case that does not hold them gets 4 x the error of the same restatement evaluated in fp32 by torch on the CPU against
# the float64 one, measured on that case (profiles/ucc_forms_tau.txt): (B, C, H, W) -> {quantity: bar}.
_TAU = {}


def _planted(B, C, H, W):
    gen = torch.Generator().manual_seed(B * 131 + C * 17 + H * 3 + W)
    N = 3 * B
    z1, z2 = (torch.randn(N, C, H, W, generator=gen) * 2 for _ in range(2))
    # planted exact ties: the top value repeated at a higher class index (pixel 0 of every row), and all classes equal (last pixel)
    for z in (z1, z2):
        flat = z.view(N, C, H * W)
        top = flat[:, :, 0].max(dim=1)
        flat[:, C - 1, 0] = top.values
        flat[:, :, H * W - 1] = 0.25
    y = torch.randint(0, C, (B, H, W), generator=gen)
    return z1, z2, y


def _restated(z1, z2, y, B, p1, p2, w, dtype):
    d1, d2 = z1.to(dtype).requires_grad_(True), z2.to(dtype).requires_grad_(True)
    r = _ucc64(d1, d2, y, B, p1, p2)
    (w[0] * r["sup"] + w[1] * r["ps"]).backward()
    return r, d1.grad, d2.grad


@pytest.mark.parametrize("B,C,H,W", _SWEEP)
def test_ucc_kernels_vs_float64(B, C, H, W):
    """Both code paths (H W % 4 == 0: four pixels a lane; otherwise one), every class count the dispatch builds at its ends and in the
    middle, one and several blocks.  The float64 side takes its arg-max over the same fp32 logits, so the pseudo-labels must be
    bit-equal.  Bounds as test_cps_kernels_vs_float64 (1e-5; see _TAU); the only new error source is fp32 exp / log around
    exp(-v), v up to ~10."""
    from uaps_amd import ucc
    z1, z2, y = _planted(B, C, H, W)
    p1, p2 = _argmax_first(z2[B:2 * B]), _argmax_first(z1[B:2 * B])
    assert bool((p1.view(B, -1)[:, -1] == 0).all()) and bool((p2.view(B, -1)[:, -1] == 0).all())
    w = (0.83, 0.57)
    ref, r1, r2 = _restated(z1, z2, y, B, p1, p2, w, torch.float64)
    tau = {"terms": 1e-5, "var": 1e-5, "grad": 1e-5, "sum": 1e-5, **_TAU.get((B, C, H, W), {})}
    g1, g2 = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    out = ucc.ucc_loss(g1, g2, y.to(DEV), B, return_var=True)
    (w[0] * out[0] + w[1] * out[1]).backward()
    sc = ucc.ucc_scalars(out[2], C)
    assert torch.equal(out[3].cpu().long(), p1) and torch.equal(out[4].cpu().long(), p2)          # ties -> the lowest index
    fig = {"terms": 0.0, "var": 0.0, "grad": 0.0, "sum": 0.0}
    pairs = [(sc["ce"][i], ref["ce"][i]) for i in range(4)] + [(sc["dice"][i], ref["dice"][i]) for i in range(4)] + \
            [(out[0], ref["sup"]), (out[1], ref["ps"]), (sc["ps_1"], ref["ps_1"]), (sc["ps_2"], ref["ps_2"]),
             (sc["v1"], ref["v1"].mean()), (sc["v2"], ref["v2"].mean())]
    for got, want in pairs:
        fig["terms"] = max(fig["terms"], abs(float(got) - float(want)) / abs(float(want)))
    for got, want in ((out[5], ref["v1"]), (out[6], ref["v2"])):
        fig["var"] = max(fig["var"], float((got.cpu().double() - want.detach()).abs().max()) / float(want.abs().max()))
    for got, want in ((g1.grad, r1), (g2.grad, r2)):
        scale = float(want.abs().max())
        fig["grad"] = max(fig["grad"], float((got.cpu().double() - want).abs().max()) / scale)
        fig["sum"] = max(fig["sum"], float(got.sum(dim=1).abs().max()) / scale)
    print(f"ucc sweep {(B, C, H, W)}: " + " ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v <= tau[k], (k, v, tau[k])
    # two runs give the same bits
    h1, h2 = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    again = ucc.ucc_loss(h1, h2, y.to(DEV), B, return_var=True)
    (w[0] * again[0] + w[1] * again[1]).backward()
    assert torch.equal(again[2], out[2]) and torch.equal(h1.grad, g1.grad) and torch.equal(h2.grad, g2.grad)
    assert torch.equal(again[5], out[5]) and torch.equal(again[6], out[6])


@pytest.mark.parametrize("H,W", [(16, 24), (37, 53)])
def test_ucc_bwd_overwrites_every_row_and_null_scales_mean_one(H, W):
    from uaps_amd import _lib, ucc
    gen = torch.Generator().manual_seed(5)
    z1, z2 = (torch.randn(6, 4, H, W, generator=gen).to(DEV) for _ in range(2))
    y = torch.randint(0, 4, (2, H, W), generator=gen).to(DEV)
    scalars = ucc._fwd(z1, z2, y, 2, want_pseudo=False)[0]
    one = torch.ones((), device=DEV)
    a1, a2 = torch.full_like(z1, 7.0), torch.full_like(z2, 7.0)
    ucc._bwd(z1, z2, y, 2, scalars, one, one, a1, a2)
    b1, b2 = torch.full_like(z1, -3.0), torch.full_like(z2, -3.0)
    rc = _lib.lib().uaps_ucc_bwd(z1.data_ptr(), z2.data_ptr(), y.data_ptr(), scalars.data_ptr(), None, None, 2, 4, H, W,
                                 b1.data_ptr(), b2.data_ptr(), _lib.current_stream(z1.device))
    assert rc == 0
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    assert float(a1.abs().max()) < 1.0 and float(a2.abs().max()) < 1.0


# ---- 4. the network ------------------------------------------------------------------------------------------------------------------------

def _noise_pert(noise, B):
    """`perturbations` of UNet_UAPS.forward / forward_groups: the FeatureNoise draw of group g at level i = noise[g][i]."""
    from uaps_amd import perturb

    def apply(fs):
        return [torch.cat([perturb.feature_noise_with(f[g * B:(g + 1) * B].contiguous(), noise[g][i]) for g in range(len(noise))])
                for i, f in enumerate(fs)]
    return [apply]


def _ucc_net(C=4, seed=0):
    from uaps_amd import unet
    torch.manual_seed(seed)
    return unet.UNet_UAPS(3, C, n_aux=1, dropout=[0.0] * 5)


def test_unet_uaps_forward_groups_matches_three_separate_forwards():
    """Tolerance of test_forward_groups_matches_three_separate_forwards; the noise draws injected, the running statistics checked."""
    from uaps_amd import unet
    B, H, W = 2, 64, 64
    net = _ucc_net(seed=12).to(DEV).train()
    sep = copy.deepcopy(net)
    xs = [torch.randn(B, 3, H, W, device=DEV) for _ in range(3)]
    noise = [[torch.empty(c, H >> i, W >> i, device=DEV).uniform_(-0.3, 0.3) for i, c in enumerate(unet.FEATURE_CHANNELS)] for _ in range(3)]
    with torch.no_grad():
        got = net.forward_groups(torch.cat(xs), 3, perturbations=_noise_pert(noise, B))
        refs = [sep(x, perturbations=_noise_pert([noise[g]], B)) for g, x in enumerate(xs)]
    assert len(got) == 2 and got[0].shape == (3 * B, 4, H, W)
    for d in range(2):
        ref = torch.cat([r[d] for r in refs])
        assert float((got[d] - ref).abs().max()) <= 2e-4 * float(ref.abs().max()), d
    for (n, a), (_, b) in zip(net.named_buffers(), sep.named_buffers()):
        if a.is_floating_point():
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6, msg=n)
        else:
            assert torch.equal(a, b), n
    with pytest.raises(ValueError):
        net.forward_groups(torch.cat(xs), 4)
    # the fused fan-out path (no injected draws) takes three groups too
    with torch.no_grad():
        free = net.forward_groups(torch.cat(xs), 3)
    assert free[1].shape == (3 * B, 4, H, W) and bool(torch.isfinite(free[1]).all())


def test_unet_ucc_eval_forward_matches_the_reference_fixture():
    """The tolerance tests/test_res_uaps.py uses for GPU forwards against a CPU-generated fixture."""
    import uaps_amd
    from formula_weights import formula_state_dict
    g = np.load(GOLD)
    net = uaps_amd.net_factory("unet_ucc", 3, 4)
    net.load_state_dict(formula_state_dict(net.state_dict()))
    net.to(DEV).eval()
    with torch.no_grad():
        main = net(torch.tensor(g["x"], device=DEV))[0]
    ref = g["main_seg"]
    np.testing.assert_allclose(main.cpu().numpy(), ref, rtol=2e-3, atol=2e-4 * np.abs(ref).max())


# ---- 5. a whole step against a float64 oracle -------------------------------------------------------------------------------------------------

def _sd(model, dtype):
    sd = {k: (v.detach().cpu().clone().to(dtype) if v.is_floating_point() else v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    for k in sd:
        if k.endswith(".weight") or k.endswith(".bias"):
            sd[k].requires_grad_(True)
    return sd


def _heads_of(xs, sd, noise):
    """The two heads' logits of the three forwards (UCC_unet.py:261-270), one after the other: ([3B,...], [3B,...])."""
    from oracle import uaps_oracle as O
    z1, z2 = [], []
    for x, ns in zip(xs, noise):
        f = O.encoder_forward(x, sd, "encoder", True, dropout=[0.0] * 5)
        z1.append(O.decoder_forward(f, sd, "main_decoder", True))
        z2.append(O.decoder_forward([O.feature_noise(t, n.to(t.dtype)) for t, n in zip(f, ns)], sd, "aux_decoder1", True))
    return torch.cat(z1), torch.cat(z2)


@pytest.mark.parametrize("iter_num", [0, 12000])
def test_ucc_step_vs_float64_oracle(iter_num):
    """test_cps_step_vs_float64_oracle for UCC: dropout zero, the FeatureNoise draws injected per group, forced rectangles with a flag
    set in each list, out_conv x 8 for confident logits.  The rule of tests/test_gpu_cct_dct.py's _compare: the loss terms to 2e-5,
    every gradient to max(5e-3 of its scale, 1e-5), the Adam update of the surely non-zero elements (|g| > max(1e-5, 1e-2 scale)) to
    0.02 lr, more than 10000 such elements.

    Pseudo-labels are discrete: the oracle's loss is evaluated with the labels the HIP step returned, and how far those may be from
    the oracle's own arg-max is bounded from the reference side alone.  The same oracle runs once more in float32 on the CPU: n32 =
    pixels whose arg-max differs from the float64 run, e32 = the largest |logit difference| of the two runs (weak rows, both heads).
    The HIP labels may differ from the float64 arg-max at no more than 4 n32 + 4 pixels, and only where the float64 top-2 logit gap
    is below 16 e32.
    Measured on MI355X (also in DESIGN.md section 3.13): iter 0: n32 = 0, e32 = 2.2e-5, HIP labels off the float64 arg-max at 0 of
    16384 pixels; iter 12000: n32 = 0, e32 = 2.4e-5, 0 pixels."""
    import uaps_amd
    from uaps_amd import unet
    from uaps_amd.ramps import get_current_consistency_weight
    rng = np.random.default_rng(71 + iter_num)
    B, C, H, W = 2, 4, 64, 64
    model = _ucc_net(C, seed=81)
    with torch.no_grad():
        for dec in (model.main_decoder, model.aux_decoder1):
            dec.out_conv.weight.mul_(8.0)
    x_l, x_wk, x_st = (torch.tensor(rng.standard_normal((B, 3, H, W)).astype(np.float32)) for _ in range(3))
    y_l = torch.tensor(uaps_amd.data.synthetic_masks(rng, B, C, H, W))
    noise = [[torch.tensor(rng.uniform(-0.3, 0.3, (c, H >> i, W >> i)).astype(np.float32)) for i, c in enumerate(unet.FEATURE_CHANNELS)]
             for _ in range(3)]
    rl = np.array([(1, 8, 40, 4, 50), (0, 0, 32, 0, 64)], dtype=np.int32)
    ru = np.array([(0, 10, 42, 10, 42), (1, 20, 64, 0, 33)], dtype=np.int32)
    cw = get_current_consistency_weight(0.1, iter_num, 200, 150)
    init = {k: v.detach().clone() for k, v in model.named_parameters()}
    mixed, y_mix = _cutmix_where(x_l, y_l, x_wk, x_st, rl, ru)
    xs = [mixed[:B], mixed[B:2 * B], mixed[2 * B:]]
    # ---- the oracle's logits in float64 and in float32 ----
    sd = _sd(model, torch.float64)
    z64 = _heads_of([x.double() for x in xs], sd, noise)
    with torch.no_grad():
        z32 = _heads_of(xs, _sd(model, torch.float32), noise)
    wk = slice(B, 2 * B)
    am64 = [_argmax_first(z64[1][wk]), _argmax_first(z64[0][wk])]                  # pseudo_1 from head 2, pseudo_2 from head 1
    am32 = [_argmax_first(z32[1][wk]), _argmax_first(z32[0][wk])]
    n32 = sum(int((a != b).sum()) for a, b in zip(am32, am64))
    e32 = max(float((a[wk].double() - b[wk].detach()).abs().max()) for a, b in zip(z32, z64))
    # ---- the HIP step ----
    model.to(DEV)
    pert = _noise_pert([[n.to(DEV) for n in ns] for ns in noise], B)
    orig = model.forward_groups
    model.forward_groups = lambda b, g, perturbations=None: orig(b, g, perturbations=pert)
    tr = uaps_amd.UCCTrainer(model, base_lr=1e-3)
    tr.iter_num = iter_num
    captured = {}
    hooks = [p.register_hook(lambda g, n=n: captured.__setitem__(n, g.detach().clone())) for n, p in model.named_parameters()]
    res = tr.train_step(x_l.to(DEV), y_l.to(DEV), x_wk.to(DEV), x_st.to(DEV), rects=(rl, ru))
    for h in hooks:
        h.remove()
    assert res["cw"] == cw
    hip = [res["pseudo1"].cpu().long(), res["pseudo2"].cpu().long()]
    observed = 0
    for p, am, z in zip(hip, am64, (z64[1][wk], z64[0][wk])):
        ne = p != am
        top2 = torch.topk(z.detach(), 2, dim=1).values
        gap = top2[:, 0] - top2[:, 1]
        observed += int(ne.sum())
        assert not bool((ne & (gap >= 16 * e32)).any()), "a pseudo-label differs where the float64 logits are not close"
    print(f"iter {iter_num}: n32 {n32} e32 {e32:.3e} HIP labels off the float64 arg-max at {observed} of {2 * B * H * W} pixels")
    assert observed <= 4 * n32 + 4, (observed, n32)
    # ---- the float64 loss with the HIP step's labels, autograd, Adam ----
    r = _ucc64(z64[0], z64[1], y_mix, B, hip[0], hip[1])
    loss = r["sup"] + cw * r["ps"]
    loss.backward()
    for key, ref in (("ce", (r["ce"][0] + r["ce"][1]) / 2), ("dice", (r["dice"][0] + r["dice"][1]) / 2), ("ps", r["ps"]), ("ps_1", r["ps_1"]),
                     ("ps_2", r["ps_2"]), ("sup", r["sup"]), ("loss", loss)):
        np.testing.assert_allclose(float(res[key]), float(ref), rtol=2e-5, err_msg=key)
    np.testing.assert_allclose(float(res["unsup"]), float(cw * r["ps"]), rtol=2e-5, atol=1e-12)
    pkeys = [k for k in sd if sd[k].requires_grad and sd[k].grad is not None]
    grads = {k: sd[k].grad.clone() for k in pkeys}
    torch.optim.Adam([sd[k] for k in pkeys], lr=1e-3).step()
    checked = 0
    for n, p in model.named_parameters():
        g_ref = grads[n]
        scale = float(g_ref.abs().max())
        err = float((captured[n].cpu().double() - g_ref).abs().max())
        assert err <= max(5e-3 * scale, 1e-5), f"{n}: max err {err:.3e} vs scale {scale:.3e}"
        sure = g_ref.abs() > max(1e-5, 1e-2 * scale)
        delta, delta_ref = p.detach().cpu() - init[n], (sd[n].detach() - init[n].double()).float()
        checked += int(sure.sum())
        if sure.any():
            assert float((delta[sure] - delta_ref[sure]).abs().max()) <= 0.02 * 1e-3, n
    assert checked > 10000


# ---- 6. trainer behaviour ------------------------------------------------------------------------------------------------------------------

def _ucc_trainer(seed=5, **kw):
    import uaps_amd
    torch.manual_seed(seed)
    return uaps_amd.UCCTrainer(uaps_amd.net_factory("unet_ucc", 3, 4).to(DEV), **kw)


def _items(n):
    import uaps_amd
    data = uaps_amd.data.SyntheticBatches(2, H=64, W=64, n_batches=n, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(3)
    return [(xl, yl, xu, xu + 0.3 * torch.randn(xu.shape, device=DEV, generator=gen)) for xl, yl, xu in data.items]


def test_one_step_moves_the_encoder_and_both_decoders():
    tr = _ucc_trainer()
    before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
    res = tr.train_step(*_items(1)[0])
    for key in ("loss", "ce", "dice", "ps", "ps_1", "ps_2", "sup", "unsup"):
        assert torch.is_tensor(res[key]) and res[key].is_cuda and bool(torch.isfinite(res[key])), key
    assert isinstance(res["cw"], float) and res["pseudo1"].dtype == torch.uint8 and res["pseudo1"].shape == (2, 64, 64)
    for part in ("encoder", "main_decoder", "aux_decoder1"):
        moved = sum(int(not torch.equal(p, before[n])) for n, p in tr.model.named_parameters() if n.startswith(part))
        assert moved > 10, part
    assert tr.iter_num == 1
    m1, m2 = tr.epoch_metrics(), tr.epoch_metrics2()
    assert np.isfinite(m1["mdice"]) and np.isfinite(m2["mdice"])


def test_checkpoint_round_trip_resumes_bit_identically(tmp_path):
    items = _items(3)
    a = _ucc_trainer()
    a.train_step(*items[0])
    a.train_step(*items[1])
    path = str(tmp_path / "ucc.pth")
    a.save_checkpoint(path, 1, 0.5)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    for k in ("epoch", "best_dice_1", "state_dict", "optimizer", "perturb_rng", "np_global_rng", "cut_np_rng", "cut_py_rng", "iter_num",
              "scheduler"):
        assert k in ck, k
    assert list(ck["state_dict"])[0].startswith("encoder.")                  # the bare model: no `module.` prefix
    ra = a.train_step(*items[2])
    b = _ucc_trainer(seed=77)
    b.load_checkpoint(path)
    assert b.iter_num == 2
    rb = b.train_step(*items[2])                                             # draws the same rectangles as `a` did
    for key in ("loss", "ce", "dice", "ps", "ps_1", "ps_2", "sup"):
        assert torch.equal(ra[key], rb[key]), key
    assert torch.equal(ra["pseudo1"], rb["pseudo1"]) and torch.equal(ra["pseudo2"], rb["pseudo2"])
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), n


def test_fit_two_short_epochs_on_four_tuple_items_writes_the_references_checkpoint(tmp_path):
    items = _items(2)
    lab = [(xl, yl) for xl, yl, _, _ in items]
    unl = [(wk, st, yl, yl) for _, yl, wk, st in items]                      # (inputs_U1, inputs_U2, labels_U1, labels_U2), :147
    tr = _ucc_trainer(seed=6)
    path = str(tmp_path / "run" / "UCC.pth")
    hist = tr.fit(lab, unl, lab, epochs=3, iter_per_epoch=3, checkpoint_path=path)
    assert len(hist) == 2 and tr.iter_num == 4
    for rec in hist:
        for k in ("loss", "ce", "dice", "ps", "ps_1", "ps_2", "sup", "unsup", "cw", "val_mdice", "val_ce", "val_loss", "lr", "train_mdice"):
            assert np.isfinite(rec[k]), k
    assert hist[0]["saved"]                                                  # the first validation beats the initial best of 0
    ck = torch.load(path, map_location="cpu", weights_only=True)
    for k in ("epoch", "best_dice_1", "state_dict", "optimizer"):
        assert k in ck, k
    assert ck["best_dice_1"] == tr.best_dice[0] and not any(k.startswith("module.") for k in ck["state_dict"])


def _kernel_counts(step):
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return {e.key: e.count for e in prof.key_averages()}


def test_one_step_launches_each_ucc_kernel_once_and_no_aten_softmax_argmax_nll_cat_or_where():
    item = _items(1)[0]
    tr = _ucc_trainer(seed=7)
    counts = _kernel_counts(lambda: tr.train_step(*item))
    assert any("ucc_fwd_kernel" in n for n in counts), "the profiler recorded no device kernels of this package"
    for name in ("ucc_cutmix_kernel", "ucc_fwd_kernel", "ucc_finalize", "ucc_bwd_kernel"):
        assert sum(c for n, c in counts.items() if name in n) == 1, name
    bad = {n: c for n, c in counts.items()
           if "at::" in n and any(s in n.lower() for s in ("softmax", "argmax", "nll", "catarray", "where"))}
    assert not bad, bad
