"""The binary (one-channel sigmoid) family on the GPU: the kernels of csrc/loss_binary.hip through the C ABI and through the Python
surface against the float64 restatement of tests/binloss_ref.py over its case table, planted mistakes against the same bars, the
exactness properties (confusion counts, bit-identical repeats, untouched guard floats), the reference fixture g12_binary.npz, the
sigmoid consistency pair, a one-output-channel convolution on the HIP path, and BinaryTrainer on net_factory("unet", class_num=1)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import binloss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_binary.npz")
GUARD = 8                      # floats behind every output that must keep their value
CASES = R.cases()
_ref_cache = {}


def _reference(case):
    """(z, t, float64 reference) of a case, computed once and shared."""
    hit = _ref_cache.get(case.name)
    if hit is None:
        z, t = R.make_inputs(case)
        hit = _ref_cache[case.name] = (z, t, R.reference(case, z, t))
    return hit


def _params(case, soft):
    from uaps_amd import _lib
    p = _lib.BinLossParams()
    p.struct_size, p.terms, p.target_float = C.sizeof(_lib.BinLossParams), 127, int(soft)
    for i, k in enumerate(R.TERMS):
        p.coef[i] = R.COEFS[k]
    p.has_pos_weight, p.pos_weight = int(case.pos_weight is not None), case.pos_weight or 1.0
    p.focal_alpha, p.focal_gamma, p.focal_mean, p.beta, p.eps = 0.8, case.gamma, 1, R.BETA, 1e-7
    p.tversky_alpha, p.tversky_beta = R.TVERSKY
    return p


def _placed(host, offset, fill=None):
    """`host` (or an uninitialised run of its size) on the device `offset` floats behind a 16-byte boundary, GUARD floats of 777
    behind it; returns (the window, the whole buffer)."""
    n = host.numel()
    buf = torch.full((offset + n + GUARD,), 777.0, dtype=torch.float32, device=DEV)
    win = buf[offset:offset + n]
    if fill is None:
        win.copy_(host.reshape(-1))
    else:
        win.fill_(fill)
    return win, buf


def run_c_abi(case, z, t):
    """Forward and backward of a case through uaps_binloss_fwd / _bwd: {terms, sums, loss, bad, dz} plus the raw outputs."""
    from uaps_amd import _lib, binary_losses as Bn
    L = _lib.lib()
    B, H, W = case.shape
    soft = t.is_floating_point()
    zd, _ = _placed(z, case.offset)
    td = t.to(DEV).contiguous()
    prm = _params(case, soft)
    need = C.c_size_t()
    assert L.uaps_binloss_workspace_bytes(B, H, W, C.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    sc, sc_buf = _placed(torch.empty(_lib.BIN_NSCALARS), 0, fill=float("nan"))
    dz, dz_buf = _placed(z, case.offset, fill=float("nan"))
    grad = None if case.grad is None else torch.tensor([case.grad], dtype=torch.float32, device=DEV)
    st = _lib.current_stream(torch.device(DEV))
    assert L.uaps_binloss_fwd(zd.data_ptr(), td.data_ptr(), C.byref(prm), B, H, W, sc.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
    assert L.uaps_binloss_bwd(zd.data_ptr(), td.data_ptr(), C.byref(prm), sc.data_ptr(), grad.data_ptr() if grad is not None else None,
                              B, H, W, dz.data_ptr(), st) == 0
    torch.cuda.synchronize()
    s = sc.cpu().double().numpy()
    got = {k: s[Bn.S_OFF["term"] + i] for i, k in enumerate(R.TERMS)}
    got.update({k: s[Bn.S_OFF[k]] for k in ("loss", "bad") + R.SUMS})
    got["dz"] = dz.cpu().double().numpy()
    return got, (sc_buf, dz_buf, case.offset + z.numel())


def run_python(case, z, t):
    from uaps_amd import binary_losses as Bn
    crit = Bn.BinarySegLoss(R.COEFS, pos_weight=case.pos_weight, focal_gamma=case.gamma, beta=R.BETA, tversky=R.TVERSKY)
    zd = z.to(DEV).requires_grad_(True)
    out = crit(zd, t.to(DEV))
    (out.loss * (1.0 if case.grad is None else case.grad)).backward()
    sc = {k: float(v) for k, v in Bn.bin_scalars(out.scalars).items()}
    sc["dz"] = zd.grad.cpu().double().reshape(-1).numpy()
    return sc


# ---- 1. the case table against float64 -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_binloss_kernels_vs_float64_through_the_c_abi(case):
    z, t, ref = _reference(case)
    got, (sc_buf, dz_buf, n_dz) = run_c_abi(case, z, t)
    err = R.errors(got, ref)
    print(case.name, " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    for k in R.QUANTITIES:
        assert err[k] <= R.TAU[k], (case.name, k, err[k], R.TAU[k])
    assert got["bad"] == (2 if case.target == "bad2" else 0)
    assert got["n"] == z.numel() - got["bad"]
    if case.target == "bad2":
        flat = got["dz"]
        assert flat[3] == 0 and flat[flat.size - 2] == 0
    assert np.isfinite(got["dz"]).all()
    # guard floats behind the scalars and behind dz keep their value
    from uaps_amd import _lib
    assert bool((sc_buf[_lib.BIN_NSCALARS:] == 777.0).all()) and bool((dz_buf[n_dz:] == 777.0).all())
    assert bool((dz_buf[:case.offset] == 777.0).all())


@pytest.mark.parametrize("case", [c for c in CASES if c.offset == 0], ids=[c.name for c in CASES if c.offset == 0])
def test_binary_seg_loss_vs_float64_through_the_python_surface(case):
    z, t, ref = _reference(case)
    got = run_python(case, z, t)
    err = R.errors(got, ref)
    for k in R.QUANTITIES:
        assert err[k] <= R.TAU[k], (case.name, k, err[k], R.TAU[k])
    assert got["bad"] == (2 if case.target == "bad2" else 0)


PLANTED = {"no_pos_weight": ("3x33x19-posw", ("bce", "loss", "dz")), "detached_pt": ("3x33x19-g15", ("dz",)),
           "ineg_without_i": ("3x33x19-int", ("dice2", "jaccard2", "tversky2", "loss", "dz")), "no_pq": ("3x33x19-int", ("dz",))}


@pytest.mark.parametrize("plant", R.PLANTS)
def test_the_bars_catch_planted_mistakes(plant):
    """The float64 reference with ONE mistake planted lies outside the bars around the kernels' result, in the quantities the mistake
    touches: a sweep that passes cannot be hiding it."""
    name, touched = PLANTED[plant]
    case = next(c for c in CASES if c.name == name)
    z, t, _ = _reference(case)
    got, _ = run_c_abi(case, z, t)
    wrong = R.reference(case, z, t, planted=plant)
    err = R.errors(got, wrong)
    print(plant, " ".join(f"{k} {err[k]:.2e}" for k in touched))
    for k in touched:
        assert err[k] > 10 * R.TAU[k], (plant, k, err[k], R.TAU[k])


# ---- 2. exactness ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 33, 19), (2, 96, 100), (3, 512, 512)])
@pytest.mark.parametrize("thr", [0.5, 0.3])
def test_bin_confusion_is_exact(shape, thr):
    from uaps_amd import binary_losses as Bn
    rng = np.random.default_rng(7)
    B, H, W = shape
    z = (rng.standard_normal((B, 1, H, W)) * 2).astype(np.float32)
    z.reshape(-1)[:4] = [0.0, float(Bn.logit_cut(thr)), np.nextafter(Bn.logit_cut(thr), np.float32(9)), -0.0]      # on and beside the cut
    y = (rng.random((B, H, W)) < 0.3).astype(np.int64)
    y.reshape(-1)[5], y.reshape(-1)[-1] = 4, -2                                     # not counted
    pred = (z.reshape(-1) > Bn.logit_cut(thr)).astype(np.int64)
    yy = y.reshape(-1)
    ok = (yy == 0) | (yy == 1)
    want = np.bincount((2 * yy + pred)[ok], minlength=4).reshape(2, 2)
    out = torch.full((2, 2 + 2), -5, dtype=torch.int64, device=DEV)                 # [2][2] + guard
    flat = out.view(-1)
    got = Bn.bin_confusion(torch.tensor(z, device=DEV), torch.tensor(y, device=DEV), thr, out=flat[:4].view(2, 2))
    assert got.dtype == torch.int64 and (got.cpu().numpy() == want).all(), (got, want)
    assert int(got.sum()) == z.size - 2 and bool((flat[4:] == -5).all())


@pytest.mark.parametrize("name", ["2x96x100-float-posw-g15", "3x512x512-int", "1x1x403-off1-float"])
def test_a_second_launch_gives_the_same_bits(name):
    case = next(c for c in CASES if c.name == name)
    z, t, _ = _reference(case)
    a, _ = run_c_abi(case, z, t)
    b, _ = run_c_abi(case, z, t)
    for k in R.TERMS + R.SUMS + ("loss",):
        assert a[k] == b[k], k
    assert np.array_equal(a["dz"], b["dz"])


def test_bwd_with_a_null_gradient_is_a_unit_gradient_and_one_term_alone_is_its_own_loss():
    from uaps_amd import binary_losses as Bn
    case = next(c for c in CASES if c.name == "3x33x19-posw")
    z, t, ref = _reference(case)
    zd = z.to(DEV).requires_grad_(True)
    for k in R.TERMS:
        crit = Bn.BinarySegLoss({k: 1.0}, pos_weight=case.pos_weight, focal_gamma=case.gamma, beta=R.BETA, tversky=R.TVERSKY)
        out = crit(zd, t.to(DEV))
        sc = Bn.bin_scalars(out.scalars)
        assert float(out.loss) == float(sc[k]) and all(float(sc[o]) == 0 for o in R.TERMS if o != k)
        assert abs(float(out.loss) - ref[k]) <= R.TAU[k] * max(abs(ref[k]), 1e-3)


# ---- 3. the reference's fixture and the consistency pair -------------------------------------------------------------------------------

def test_binary_losses_match_the_reference_fixture_on_the_gpu():
    assert R.check_fixture(np.load(GOLD), DEV) > 60


@pytest.mark.parametrize("name", ["3x33x19-int", "3x33x19-zeros"])
def test_unthresholded_iou_and_f_score_keep_their_digits_and_their_gradient(name):
    """iou / f_score without a threshold come from the forward's sums, not from 1 - loss: at an all-background target the score is
    eps / (P + eps) ~ 1e-10, which 1 - fp32(loss) rounds to 0.  Value at the fixture bar (1e-4 relative), gradient 1e-4 of max|g|."""
    from uaps_amd import binary_losses as Bn
    case = next(c for c in CASES if c.name == name)
    z, t, _ = _reference(case)
    for fn, kw in ((Bn.iou, {}), (Bn.f_score, {"beta": 1.5})):
        zd, z64 = z.to(DEV).requires_grad_(True), z.double().requires_grad_(True)
        got = fn(zd, t.to(DEV), **kw)
        terms = R.bin_terms(t, z64, beta=1.5)
        want = 1 - terms["jaccard" if fn is Bn.iou else "fscore"]
        if name.endswith("zeros"):                               # 1 - (1 - tiny) has no digits in float64 either: the closed form
            want = 1e-7 / (terms["P"] + 1e-7)
        got.backward()
        want.backward()
        got, want = float(got.detach()), float(want.detach())
        assert got > 0 and abs(got - want) <= 1e-4 * want, (name, fn.__name__, got, want)
        g64 = z64.grad.reshape(-1)
        assert float((zd.grad.cpu().double().reshape(-1) - g64).abs().max()) <= 1e-4 * float(g64.abs().max())


PAIR_SHAPES = [((1, 1, 5, 7), 0), ((3, 1, 33, 19), 0), ((2, 1, 96, 100), 0), ((1, 1, 1, 403), 1), ((3, 1, 512, 512), 0)]


def pair_inputs(shape):
    rng = np.random.default_rng(21)
    n = int(np.prod(shape))
    a = np.clip(rng.standard_normal(n) * 6, -30, 30).astype(np.float32)
    b = np.clip(rng.standard_normal(n) * 6, -30, 30).astype(np.float32)
    gm = rng.standard_normal(n).astype(np.float32)
    return torch.tensor(a), torch.tensor(b), torch.tensor(gm)


def pair_errors(a, b, gm, run):
    """Errors of the sigmoid MSE / KL pair against float64 in the quantities of R.TAU_PAIR: the map absolutely (its values lie in
    [0, 1]), the KL mean relatively, each gradient relative to max|g|.  `run(a, b, gm)` -> (map, d map, kl, d kl) as flat float64
    arrays / a float, the KL's incoming gradient being 0.7."""
    a64 = a.double().requires_grad_(True)
    m64 = R.sigmoid_mse(a64, b.double())
    m64.backward(gm.double())
    dm64, a64.grad = a64.grad.clone(), None
    k64 = R.sigmoid_kl(a64, b.double())
    (k64 * 0.7).backward()
    m, dm, k, dk = run(a, b, gm)
    return {"mse_map": float(np.abs(m - m64.detach().numpy()).max()),
            "mse_da": float(np.abs(dm - dm64.numpy()).max() / float(dm64.abs().max())),
            "kl": abs(k - float(k64)) / abs(float(k64)),
            "kl_da": float(np.abs(dk - a64.grad.numpy()).max() / float(a64.grad.abs().max()))}


def pair_float32(a, b, gm):
    """The fp32 floor: the same two losses composed from torch ops in float32 on the CPU."""
    x = a.clone().requires_grad_(True)
    m = R.sigmoid_mse(x, b)
    m.backward(gm)
    dm, x.grad = x.grad.clone(), None
    k = R.sigmoid_kl(x, b)
    (k * 0.7).backward()
    return m.detach().double().numpy(), dm.double().numpy(), float(k.detach()), x.grad.double().numpy()


def pair_kernels(offset):
    """`run` of pair_errors through the C ABI, every tensor `offset` floats behind a 16-byte boundary; keeps the whole output buffers
    for the guard check in `.guards` ([(buffer, floats in front of the output, the output's end)])."""
    def run(a, b, gm):
        from uaps_amd import _lib
        L = _lib.lib()
        n = a.numel()
        ad, bd, gd = (_placed(v, offset)[0] for v in (a, b, gm))
        (m, m_buf), (dm, dm_buf), (dk, dk_buf) = (_placed(a, offset, fill=float("nan")) for _ in range(3))
        k, k_buf = _placed(torch.empty(1), 0, fill=float("nan"))
        g07 = torch.tensor([0.7], dtype=torch.float32, device=DEV)
        need = C.c_size_t()
        assert L.uaps_binloss_workspace_bytes(1, 1, 1, C.byref(need)) == 0
        ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
        st = _lib.current_stream(torch.device(DEV))
        assert L.uaps_sigmoid_mse_fwd(ad.data_ptr(), bd.data_ptr(), n, m.data_ptr(), st) == 0
        assert L.uaps_sigmoid_mse_bwd(ad.data_ptr(), bd.data_ptr(), gd.data_ptr(), n, dm.data_ptr(), st) == 0
        assert L.uaps_sigmoid_kl_fwd(ad.data_ptr(), bd.data_ptr(), n, k.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
        assert L.uaps_sigmoid_kl_bwd(ad.data_ptr(), bd.data_ptr(), g07.data_ptr(), n, dk.data_ptr(), st) == 0
        torch.cuda.synchronize()
        run.guards = [(m_buf, offset, offset + n), (dm_buf, offset, offset + n), (dk_buf, offset, offset + n), (k_buf, 0, 1)]
        return m.cpu().double().numpy(), dm.cpu().double().numpy(), float(k.cpu()[0]), dk.cpu().double().numpy()
    return run


@pytest.mark.parametrize("shape,offset", PAIR_SHAPES)
def test_sigmoid_mse_and_kl_vs_float64(shape, offset):
    """Map, mean and both gradients through the C ABI against float64 at the bars of R.TAU_PAIR; guard floats in front of and behind
    every output keep their value; the Python surface gives the same bits, no gradient to the target, and the same KL twice."""
    from uaps_amd import binary_losses as Bn
    a, b, gm = pair_inputs(shape)
    run = pair_kernels(offset)
    err = pair_errors(a, b, gm, run)
    print(shape, offset, " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    for k, v in err.items():
        assert v <= R.TAU_PAIR[k], (k, v, R.TAU_PAIR[k])
    for buf, lead, end in run.guards:
        assert bool((buf[end:] == 777.0).all()) and bool((buf[:lead] == 777.0).all())
    m, dm, k, dk = run(a, b, gm)
    ad = _placed(a, offset)[0].view(shape).requires_grad_(True)
    bd = _placed(b, offset)[0].view(shape).requires_grad_(True)
    pm = Bn.sigmoid_mse_loss(ad, bd)
    pm.backward(gm.to(DEV).view(shape))
    assert np.array_equal(pm.detach().cpu().double().reshape(-1).numpy(), m)
    assert np.array_equal(ad.grad.cpu().double().reshape(-1).numpy(), dm) and bd.grad is None
    ad.grad = None
    pk = Bn.sigmoid_kl_loss(ad, bd)
    (pk * 0.7).backward()
    assert float(pk.detach()) == k and float(Bn.sigmoid_kl_loss(ad.detach(), bd.detach())) == k          # deterministic
    assert np.array_equal(ad.grad.cpu().double().reshape(-1).numpy(), dk) and bd.grad is None


def test_no_label_in_range_gives_zero_means_and_a_zero_gradient():
    """n == 0 (every label outside {0, 1}): bce and focal are 0, not 0 / 0; every scalar is finite; dz is 0 everywhere; the CPU
    composition defines the same values."""
    from uaps_amd import binary_losses as Bn
    z = torch.tensor(np.random.default_rng(5).standard_normal((2, 1, 9, 7)).astype(np.float32))
    y = torch.full((2, 9, 7), 5, dtype=torch.int64)
    crit = Bn.BinarySegLoss(R.COEFS, pos_weight=2.0, beta=R.BETA, tversky=R.TVERSKY)
    zd = z.to(DEV).requires_grad_(True)
    out = crit(zd, y.to(DEV))
    out.loss.backward()
    sc = {k: float(v) for k, v in Bn.bin_scalars(out.scalars).items()}
    assert bool(torch.isfinite(out.scalars).all()) and sc["bce"] == 0 and sc["focal"] == 0 and sc["n"] == 0 and sc["bad"] == z.numel()
    assert bool((zd.grad == 0).all())
    cpu = {k: float(v) for k, v in Bn.bin_scalars(crit(z, y).scalars).items()}
    for k in R.TERMS + ("loss",):
        assert abs(sc[k] - cpu[k]) <= 1e-6, (k, sc[k], cpu[k])


# ---- 4. a one-output-channel convolution and the trainer -------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(32, 32), (64, 64)])
def test_out_conv_with_one_output_channel_runs_forward_and_both_gradients_on_the_hip_path(H, W):
    """16 -> 1 channels, 3x3: forward, input gradient and weight gradient of `conv.conv2d` against F.conv2d in float64, on a map
    narrower than 64 (the tile kernels) and at 64 (the <= 4-output-channel kernels of conv_small.hpp).  Bars from the number format,
    per element: a sum of K products computed in fp32 is off by at most (K + 4) u S, u = 2^-24, S the same sum over the absolute
    values (K additions of u each; a product is exact to u in fp32 and to 4 u = 2^-22 where a two-piece fp16 split form runs), with
    K = 144 per output, 9 per input gradient and B H W per weight gradient.  S comes from the same convolution of |x|, |w|, |dy|."""
    from uaps_amd import conv
    torch.manual_seed(4)
    B = 2
    x = torch.randn(B, 16, H, W)
    w = torch.randn(1, 16, 3, 3) * 0.1
    b = torch.randn(1)
    dy = torch.randn(B, 1, H, W)
    xd, wd, bd = (v.to(DEV).requires_grad_(True) for v in (x, w, b))
    y = conv.conv2d(xd, wd, bd)
    y.backward(dy.to(DEV))
    x64, w64, b64 = (v.double().requires_grad_(True) for v in (x, w, b))
    y64 = torch.nn.functional.conv2d(x64, w64, b64, padding=1)
    y64.backward(dy.double())
    xa, wa, ba = (v.double().abs().requires_grad_(True) for v in (x, w, b))
    ya = torch.nn.functional.conv2d(xa, wa, ba, padding=1)
    ya.backward(dy.double().abs())
    u = 2.0 ** -24
    assert y.shape == (B, 1, H, W)
    for got, ref, size, K in ((y.detach(), y64.detach(), ya.detach(), 145), (xd.grad, x64.grad, xa.grad, 9),
                              (wd.grad, w64.grad, wa.grad, B * H * W), (bd.grad, b64.grad, ba.grad, B * H * W)):
        assert bool(((got.cpu().double() - ref).abs() <= (K + 4) * u * size).all()), (K, float((got.cpu().double() - ref).abs().max()))


def _sd64(model):
    sd = {k: (v.detach().cpu().clone().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    for k in sd:
        if k.endswith(".weight") or k.endswith(".bias"):
            sd[k].requires_grad_(True)
    return sd


def _binary_unet():
    import uaps_amd
    torch.manual_seed(41)
    model = uaps_amd.net_factory("unet", 3, 1)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model.to(DEV)


def test_binary_trainer_step_vs_a_float64_step():
    """One BinaryTrainer.train_step of net_factory("unet", class_num=1) at 2 x 3 x 32 x 32 against a float64 CPU run of the same
    model (oracle.uaps_oracle's network) and criterion (tests/binloss_ref.py).  The bars of the existing step tests
    (test_baseline_trainer_steps_with_a_segloss_vs_float64_steps): loss and terms rtol 2e-5, every gradient max(5e-3 of its scale, 1e-5)."""
    import uaps_amd
    from oracle import uaps_oracle as O
    rng = np.random.default_rng(41)
    B, H, W = 2, 32, 32
    model = _binary_unet()
    tr = uaps_amd.BinaryTrainer(model, base_lr=1e-3)
    x = torch.tensor(rng.standard_normal((B, 3, H, W)).astype(np.float32))
    y = torch.tensor((uaps_amd.data.synthetic_masks(rng, B, 2, H, W) > 0).astype(np.int64))
    sd = _sd64(model)
    logits = O.decoder_forward(O.encoder_forward(x.double(), sd, "encoder", True, dropout=[0.0] * 5), sd, "decoder", True)
    assert logits.shape == (B, 1, H, W)
    terms = R.bin_terms(y, logits)
    loss = 0.6 * terms["bce"] + 0.4 * terms["fscore"]
    loss.backward()
    captured = {}
    hooks = [p.register_hook(lambda g, n=n: captured.__setitem__(n, g.detach().clone())) for n, p in model.named_parameters()]
    res = tr.train_step(x.to(DEV), y.to(DEV))
    for h in hooks:
        h.remove()
    assert set(res) == {"loss", "bce", "fscore", "bad_labels"} and float(res["bad_labels"]) == 0.0
    for key, ref in (("loss", loss), ("bce", terms["bce"]), ("fscore", terms["fscore"])):
        np.testing.assert_allclose(float(res[key]), float(ref.detach()), rtol=2e-5, err_msg=key)
    checked = 0
    for n, p in model.named_parameters():
        g_ref = sd[n].grad
        scale = float(g_ref.abs().max())
        err = float((captured[n].cpu().double() - g_ref).abs().max())
        assert err <= max(5e-3 * scale, 1e-5), f"{n}: max err {err:.3e} vs scale {scale:.3e}"
        checked += g_ref.numel()
    assert checked > 10000 and tr.iter_num == 1
    assert tuple(captured["decoder.out_conv.weight"].shape) == (1, 16, 3, 3)
    cm = tr._cms[0].cpu().numpy()
    assert cm.shape == (2, 2) and cm.sum() == B * H * W


def test_binary_trainer_learns_validates_and_round_trips_its_checkpoint(tmp_path):
    import uaps_amd
    rng = np.random.default_rng(43)
    B, H, W = 2, 32, 32
    model = _binary_unet()
    tr = uaps_amd.BinaryTrainer(model, base_lr=1e-3, threshold=0.4)
    x = torch.tensor(rng.standard_normal((B, 3, H, W)).astype(np.float32), device=DEV)
    y = torch.tensor((uaps_amd.data.synthetic_masks(rng, B, 2, H, W) > 0).astype(np.int64), device=DEV)
    losses = [float(tr.train_step(x, y)["loss"]) for _ in range(3)]
    assert losses[2] < losses[0], losses
    train = tr.epoch_metrics()
    assert set(train) == {"miou", "mdice", "acc"} and 0 <= train["acc"] <= 1
    val = tr.validate([(x, y), (x.flip(3), y.flip(2))])
    for k in ("iou", "dice", "miou", "mdice", "acc", "ce", "loss"):
        assert np.isfinite(val[k]), (k, val)
    path = str(tmp_path / "binary.pth")
    tr.save_checkpoint(path, epoch=3, best_dice=val["mdice"])
    other = uaps_amd.BinaryTrainer(_binary_unet(), base_lr=1e-3, threshold=0.4)
    for p in other.model.parameters():
        p.data.add_(0.5)
    ck = other.load_checkpoint(path)
    assert ck["epoch"] == 3 and other.iter_num == 3
    for (n, a), (_, b) in zip(model.state_dict().items(), other.model.state_dict().items()):
        assert torch.equal(a, b), n
    again = other.validate([(x, y), (x.flip(3), y.flip(2))])
    assert again == val
