"""CPS on the GPU: the kernels of csrc/loss_cps.hip against the reference-generated fixture g9_cps.npz and against a float64
restatement of CPS/CPS_train.py:215-250 built from oracle.uaps_oracle, the UNet_f network, whole trainer steps against a float64
oracle, checkpoints, the epoch loop and the kernels one step launches."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_cps.npz")


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------------

def _cps64(z1, z2, y, b_lab, p1, p2):
    """CPS_train.py:215-245 on float64 logits with GIVEN pseudo-labels p1, p2 [N,H,W] (int64).  Returns (ce[6], dice[6], sup,
    labeled_cps, cps) in the term order of uaps_amd.cps.TERMS."""
    from oracle import uaps_oracle as O

    def pair(z, t):
        return O.cross_entropy(z, t), O.dice_loss(t.unsqueeze(1), z)
    l1, l2, u1, u2 = z1[:b_lab], z2[:b_lab], z1[b_lab:], z2[b_lab:]
    terms = [pair(l1, y), pair(l2, y), pair(l1, p2[:b_lab]), pair(l2, p1[:b_lab]), pair(u1, p2[b_lab:]), pair(u2, p1[b_lab:])]
    sup = 0.5 * (terms[0][0] + terms[0][1]) + 0.5 * (terms[1][0] + terms[1][1])
    lcps = (0.5 * terms[2][0] + 0.5 * terms[2][1]) + (0.5 * terms[3][0] + 0.5 * terms[3][1])
    cps = (0.5 * terms[4][0] + 0.5 * terms[4][1]) + (0.5 * terms[5][0] + 0.5 * terms[5][1])
    return [t[0] for t in terms], [t[1] for t in terms], sup, lcps, cps


def _argmax_first(z):
    """arg-max over the classes of fp32 logits, the lowest index among equal values (numpy's argmax returns the first)."""
    return torch.from_numpy(np.argmax(z.detach().cpu().numpy(), axis=1).astype(np.int64))


# ---- 1. the fixture of the reference ----------------------------------------------------------------------------------------------------

def test_cps_loss_matches_the_reference_fixture():
    """Tolerances of test_loss_block_full_size_vs_c_oracle (terms rtol 2e-5, gradients rtol 1e-3 / atol 2e-5 max|g|); pseudo-labels by
    the rule of tests/test_gpu_parity.py: identical wherever the reference's top-2 softmax gap exceeds 1e-5, fewer than 1e-4 of the
    pixels different overall."""
    from uaps_amd import cps
    g = np.load(GOLD)
    b_lab, cw = int(g["b_lab"]), float(g["cw"])
    z1 = torch.tensor(g["z1"], device=DEV, requires_grad=True)
    z2 = torch.tensor(g["z2"], device=DEV, requires_grad=True)
    y = torch.tensor(g["labels"], device=DEV)
    sup, lcps, cp, scalars, p1, p2 = cps.cps_loss(z1, z2, y, b_lab)
    (sup + cw * cp + cw * lcps).backward()
    sc = cps.cps_scalars(scalars, z1.shape[1])
    print("ce", sc["ce"].tolist(), "dice", sc["dice"].tolist(), "sup", float(sup), "lcps", float(lcps), "cps", float(cp))
    np.testing.assert_allclose(sc["ce"].cpu().double().numpy(), g["ce"], rtol=2e-5)
    np.testing.assert_allclose(sc["dice"].cpu().double().numpy(), g["dice"], rtol=2e-5)
    for got, key in ((sup, "sup"), (lcps, "labeled_cps"), (cp, "cps")):
        np.testing.assert_allclose(float(got), float(g[key]), rtol=2e-5, err_msg=key)
    assert float(sc["bad"]) == 0.0
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


# ---- 2. float64 sweep ---------------------------------------------------------------------------------------------------------------------

_SWEEP = [(4, C, H, W, b) for C in (2, 4, 7, 8) for H, W in ((37, 53), (1, 40), (16, 24)) for b in (1, 2, 3)] + [(32, 4, 256, 256, 16)]


@pytest.mark.parametrize("N,C,H,W,b_lab", _SWEEP)
def test_cps_kernels_vs_float64(N, C, H, W, b_lab):
    """Both code paths (H W % 4 == 0: four pixels a lane; otherwise one), every class count the dispatch builds at its ends and in the
    middle.  The float64 side takes its arg-max over the same fp32 logits, so the pseudo-labels must be bit-equal.  Bounds: fp32
    exp / log / division are a few ulp per pixel, the sums are fp32 over at most a block's pixels and double across blocks -> 1e-5
    on the terms (the bound of test_cct_consistency_vs_float64); a gradient element is a handful of fp32 operations on numbers no
    larger than the largest element -> 1e-5 of max|g|; the class sum of a pixel's gradient is <p, g> (1 - sum p) + c (sum p - 1),
    i.e. C fp32 roundings of the softmax times the element scale -> 1e-5 of max|g|."""
    from uaps_amd import cps
    gen = torch.Generator().manual_seed(N * 131 + C * 17 + H * 3 + W + b_lab)
    z1, z2 = (torch.randn(N, C, H, W, generator=gen) * 2 for _ in range(2))
    # planted exact ties: the top value repeated at a higher class index (pixel 0 of every row), and all classes equal (last pixel)
    for z in (z1, z2):
        flat = z.view(N, C, H * W)
        top = flat[:, :, 0].max(dim=1)
        flat[:, C - 1, 0] = top.values
        flat[:, :, H * W - 1] = 0.25
    y = torch.randint(0, C, (b_lab, H, W), generator=gen)
    p1, p2 = _argmax_first(z1), _argmax_first(z2)
    assert bool((p1.view(N, -1)[:, -1] == 0).all()) and bool((p2.view(N, -1)[:, -1] == 0).all())
    d1, d2 = z1.double().requires_grad_(True), z2.double().requires_grad_(True)
    ce, dice, sup, lcps, cp = _cps64(d1, d2, y, b_lab, p1, p2)
    w = (0.83, 0.31, 0.57)
    (w[0] * sup + w[1] * lcps + w[2] * cp).backward()
    g1, g2 = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    out = cps.cps_loss(g1, g2, y.to(DEV), b_lab)
    (w[0] * out[0] + w[1] * out[1] + w[2] * out[2]).backward()
    sc = cps.cps_scalars(out[3], C)
    assert torch.equal(out[4].cpu().long(), p1) and torch.equal(out[5].cpu().long(), p2)          # ties -> the lowest index
    np.testing.assert_allclose(sc["ce"].cpu().double().numpy(), [float(t) for t in ce], rtol=1e-5)
    np.testing.assert_allclose(sc["dice"].cpu().double().numpy(), [float(t) for t in dice], rtol=1e-5)
    for got, ref in ((out[0], sup), (out[1], lcps), (out[2], cp)):
        np.testing.assert_allclose(float(got), float(ref), rtol=1e-5)
    for got, ref in ((g1.grad, d1.grad), (g2.grad, d2.grad)):
        scale = float(ref.abs().max())
        err = float((got.cpu().double() - ref).abs().max())
        assert err <= 1e-5 * scale, (err, scale)
        assert float(got.sum(dim=1).abs().max()) <= 1e-5 * scale
    # two runs give the same bits
    h1, h2 = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    again = cps.cps_loss(h1, h2, y.to(DEV), b_lab)
    (w[0] * again[0] + w[1] * again[1] + w[2] * again[2]).backward()
    assert torch.equal(again[3], out[3]) and torch.equal(h1.grad, g1.grad) and torch.equal(h2.grad, g2.grad)


def test_cps_bwd_overwrites_every_row_and_null_scales_mean_one():
    from uaps_amd import _lib, cps
    gen = torch.Generator().manual_seed(5)
    z1, z2 = (torch.randn(4, 4, 16, 24, generator=gen).to(DEV) for _ in range(2))
    y = torch.randint(0, 4, (2, 16, 24), generator=gen).to(DEV)
    scalars, _, _ = cps._fwd(z1, z2, y, 2, want_pseudo=False)
    one = torch.ones((), device=DEV)
    a1, a2 = torch.full_like(z1, 7.0), torch.full_like(z2, 7.0)
    cps._bwd(z1, z2, y, 2, scalars, one, one, one, a1, a2)
    b1, b2 = torch.full_like(z1, -3.0), torch.full_like(z2, -3.0)
    rc = _lib.lib().uaps_cps_bwd(z1.data_ptr(), z2.data_ptr(), y.data_ptr(), scalars.data_ptr(), None, None, None, 4, 2, 4, 16, 24,
                                 b1.data_ptr(), b2.data_ptr(), _lib.current_stream(z1.device))
    assert rc == 0
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    assert float(a1.abs().max()) < 1.0 and float(a2.abs().max()) < 1.0


# ---- 3. the network --------------------------------------------------------------------------------------------------------------------

def _unet_f(C=4, seed=0, dropout=False):
    import uaps_amd
    torch.manual_seed(seed)
    m = uaps_amd.UNet_f(3, C)
    if not dropout:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
    return m


def test_unet_f_eval_forward_matches_the_reference_fixture():
    """The tolerance tests/test_res_uaps.py uses for GPU forwards against a CPU-generated fixture."""
    import uaps_amd
    from formula_weights import formula_state_dict
    g = np.load(GOLD)
    net = uaps_amd.net_factory("unet_f", 3, 4)
    net.load_state_dict(formula_state_dict(net.state_dict()))
    net.to(DEV).eval()
    x = torch.tensor(g["x"], device=DEV)
    with torch.no_grad():
        out = net(x)
        main = net.forward_main(x)
    assert len(out) == 9
    for i in range(4):
        ref = g[f"dp{i}"]
        np.testing.assert_allclose(out[5 + i].cpu().numpy(), ref, rtol=2e-3, atol=2e-4 * np.abs(ref).max(), err_msg=f"dp{i}")
    assert torch.equal(main, out[5])


def test_unet_f_forward_pair_equals_two_forwards():
    """Tolerance of test_forward_groups_matches_three_separate_forwards."""
    import copy
    net = _unet_f(seed=12).to(DEV).train()
    sep = copy.deepcopy(net)
    xa, xb = torch.randn(2, 3, 64, 64, device=DEV), torch.randn(2, 3, 64, 64, device=DEV)
    with torch.no_grad():
        got = net.forward_pair(xa, xb)
        ref = torch.cat([sep(xa)[5], sep(xb)[5]])
    assert got.shape == (4, 4, 64, 64)
    assert float((got - ref).abs().max()) <= 2e-4 * float(ref.abs().max())
    for (n, a), (_, b) in zip(net.named_buffers(), sep.named_buffers()):
        if a.is_floating_point():
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6, msg=n)


# ---- 4. a whole step against a float64 oracle ----------------------------------------------------------------------------------------------

def _sd(model, dtype):
    sd = {k: (v.detach().cpu().clone().to(dtype) if v.is_floating_point() else v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    for k in sd:
        if k.endswith(".weight") or k.endswith(".bias"):
            sd[k].requires_grad_(True)
    return sd


def _logits_of(x, sd):
    from oracle import uaps_oracle as O
    return O.decoder_forward(O.encoder_forward(x, sd, "encoder", True, dropout=[0.0] * 5), sd, "decoder", True)


@pytest.mark.parametrize("iter_num", [0, 12000])
def test_cps_step_vs_float64_oracle(iter_num):
    """test_cct_step_vs_float64_oracle for CPS: dropout zero, the float64 state dict, the loss terms to 2e-5, every gradient to
    max(5e-3 of its scale, 1e-5), the Adam update of the surely non-zero elements to 0.02 lr -- per network.

    Pseudo-labels are discrete: the oracle's loss is evaluated with the labels the HIP step returned, and how far those may be from
    the oracle's own arg-max is bounded from the reference side alone.  The same oracle runs once more in float32 on the CPU: n32 =
    pixels whose arg-max differs from the float64 run, e32 = the largest |logit difference| of the two runs.  The HIP labels may
    differ from the float64 arg-max at no more than 4 n32 + 4 pixels, and only where the float64 top-2 logit gap is below 16 e32 (a
    different summation order at fp32-level error, which is what the split-fp16 convolutions deliver).
    Measured on MI355X (also in DESIGN.md section 3.12): iter 0: n32 = 0, e32 = 2.9e-5, HIP labels off the float64 arg-max at 0 of
    32768 pixels; iter 12000: n32 = 0, e32 = 2.5e-5, 0 pixels.  _compare's gradient floor (1e-5) is not loosened."""
    import uaps_amd
    from uaps_amd.ramps import get_current_consistency_weight
    rng = np.random.default_rng(51 + iter_num)
    B, C, H, W = 2, 4, 64, 64
    models = [_unet_f(C, seed=61), _unet_f(C, seed=62)]
    with torch.no_grad():
        for m in models:
            m.decoder.out_conv.weight.mul_(8.0)          # confident logits (as the DCT step test)
    x_l = torch.tensor(rng.standard_normal((B, 3, H, W)).astype(np.float32))
    x_u = torch.tensor(rng.standard_normal((B, 3, H, W)).astype(np.float32))
    y_l = torch.tensor(uaps_amd.data.synthetic_masks(rng, B, C, H, W))
    cw = get_current_consistency_weight(0.1, iter_num, 200, 150)
    init = [{k: v.detach().clone() for k, v in m.named_parameters()} for m in models]
    # ---- the oracle's logits in float64 and in float32 ----
    sds = [_sd(m, torch.float64) for m in models]
    z64 = [torch.cat([_logits_of(x_l.double(), sd), _logits_of(x_u.double(), sd)]) for sd in sds]
    with torch.no_grad():
        z32 = [torch.cat([_logits_of(x_l, sd), _logits_of(x_u, sd)]) for sd in (_sd(m, torch.float32) for m in models)]
    am64 = [_argmax_first(z) for z in z64]
    n32 = sum(int((_argmax_first(a) != b).sum()) for a, b in zip(z32, am64))
    e32 = max(float((a.double() - b.detach()).abs().max()) for a, b in zip(z32, z64))
    # ---- the HIP step ----
    for m in models:
        m.to(DEV)
    tr = uaps_amd.CPSTrainer(models[0], models[1], base_lr=1e-3)
    tr.iter_num = iter_num
    captured = [{}, {}]
    hooks = [p.register_hook(lambda g, n=n, c=c: c.__setitem__(n, g.detach().clone()))
             for m, c in zip(models, captured) for n, p in m.named_parameters()]
    res = tr.train_step(x_l.to(DEV), y_l.to(DEV), x_u.to(DEV))
    for h in hooks:
        h.remove()
    assert res["cw"] == cw
    hip = [res["pseudo1"].cpu().long(), res["pseudo2"].cpu().long()]
    observed = 0
    for p, am, z in zip(hip, am64, z64):
        ne = p != am
        top2 = torch.topk(z.detach(), 2, dim=1).values
        gap = top2[:, 0] - top2[:, 1]
        observed += int(ne.sum())
        assert not bool((ne & (gap >= 16 * e32)).any()), "a pseudo-label differs where the float64 logits are not close"
    print(f"iter {iter_num}: n32 {n32} e32 {e32:.3e} HIP labels off the float64 arg-max at {observed} pixels")
    assert observed <= 4 * n32 + 4, (observed, n32)
    # ---- the float64 loss with the HIP step's labels, autograd, Adam per network ----
    ce, dice, sup, lcps, cp = _cps64(z64[0], z64[1], y_l, B, hip[0], hip[1])
    loss = sup + cw * cp + cw * lcps
    loss.backward()
    for key, ref in (("ce_1", ce[0]), ("dice_1", dice[0]), ("ce_2", ce[1]), ("dice_2", dice[1]), ("cps", cp), ("labeled_cps", lcps),
                     ("sup", sup), ("loss", loss)):
        np.testing.assert_allclose(float(res[key]), float(ref), rtol=2e-5, err_msg=key)
    np.testing.assert_allclose(float(res["unsup"]), float(cw * cp + cw * lcps), rtol=2e-5, atol=1e-12)
    for m, sd, cap, ini in zip(models, sds, captured, init):
        pkeys = [k for k in sd if sd[k].requires_grad and sd[k].grad is not None]
        grads = {k: sd[k].grad.clone() for k in pkeys}
        torch.optim.Adam([sd[k] for k in pkeys], lr=1e-3).step()
        checked = 0
        for n, p in m.named_parameters():
            if "out_conv_dp" in n:
                # the deep-supervision heads enter no loss term: no gradient, and Adam leaves them bit for bit where they were
                assert n not in cap and sd[n].grad is None and p.grad is None
                assert torch.equal(p.detach().cpu(), ini[n]), n
                continue
            g_ref = grads[n]
            scale = float(g_ref.abs().max())
            err = float((cap[n].cpu().double() - g_ref).abs().max())
            assert err <= max(5e-3 * scale, 1e-5), f"{n}: max err {err:.3e} vs scale {scale:.3e}"
            sure = g_ref.abs() > max(1e-5, 1e-2 * scale)
            delta, delta_ref = p.detach().cpu() - ini[n], (sd[n].detach() - ini[n].double()).float()
            checked += int(sure.sum())
            if sure.any():
                assert float((delta[sure] - delta_ref[sure]).abs().max()) <= 0.02 * 1e-3, n
        assert checked > 10000


# ---- 5. trainer behaviour ------------------------------------------------------------------------------------------------------------------

def _cps_trainer(seed=5, **kw):
    import uaps_amd
    torch.manual_seed(seed)
    return uaps_amd.CPSTrainer(uaps_amd.net_factory("unet_f", 3, 4).to(DEV), uaps_amd.net_factory("unet_f", 3, 4).to(DEV), **kw)


def test_two_networks_start_from_different_weights_and_both_train():
    import uaps_amd
    data = uaps_amd.data.SyntheticBatches(2, H=64, W=64, n_batches=1, device=DEV)
    tr = _cps_trainer()
    w1, w2 = tr.model.decoder.out_conv.weight.detach().clone(), tr.model2.decoder.out_conv.weight.detach().clone()
    assert not torch.equal(w1, w2)
    res = tr.train_step(*data.items[0])
    for key in ("loss", "ce_1", "dice_1", "ce_2", "dice_2", "cps", "labeled_cps", "sup", "unsup"):
        assert torch.is_tensor(res[key]) and res[key].is_cuda and bool(torch.isfinite(res[key])), key
    assert isinstance(res["cw"], float)
    assert not torch.equal(w1, tr.model.decoder.out_conv.weight) and not torch.equal(w2, tr.model2.decoder.out_conv.weight)
    assert tr.iter_num == 1


def test_learning_rates_are_per_network():
    import uaps_amd
    data = uaps_amd.data.SyntheticBatches(2, H=64, W=64, n_batches=1, device=DEV)
    tr = _cps_trainer()
    for g in tr.optimizer2.param_groups:
        g["lr"] = 0.0
    assert tr.learning_rates() == (1e-3, 0.0)
    before = [{n: p.detach().clone() for n, p in m.named_parameters()} for m in tr.models]
    tr.train_step(*data.items[0])
    moved = [sum(int(not torch.equal(p, b[n])) for n, p in m.named_parameters()) for m, b in zip(tr.models, before)]
    assert moved[0] > 50 and moved[1] == 0


def test_checkpoint_round_trip_resumes_bit_identically(tmp_path):
    import uaps_amd
    data = uaps_amd.data.SyntheticBatches(2, H=64, W=64, n_batches=3, device=DEV)
    a = _cps_trainer()
    a.train_step(*data.items[0])
    a.train_step(*data.items[1])
    path = str(tmp_path / "cps.pth")
    a.save_checkpoint(path, 1, (0.5, 0.25))
    for which, key in ((1, "best_dice_1"), (2, "best_dice_2")):
        ck = torch.load(str(tmp_path / f"cps_{which}.pth"), map_location="cpu", weights_only=True)
        for k in ("epoch", key, "state_dict", "optimizer", "perturb_rng", "np_global_rng", "iter_num", "scheduler"):
            assert k in ck, k
        assert "decoder.out_conv_dp4.weight" in ck["state_dict"]
    ra = a.train_step(*data.items[2])
    b = _cps_trainer(seed=77)
    b.load_checkpoint(path)
    assert b.best_dice == [0.5, 0.25] and b.iter_num == 2
    rb = b.train_step(*data.items[2])
    for key in ("loss", "ce_1", "dice_1", "ce_2", "dice_2", "cps", "labeled_cps", "sup"):
        assert torch.equal(ra[key], rb[key]), key
    for ma, mb in zip(a.models, b.models):
        for (n, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
            assert torch.equal(p, q), n


def test_fit_two_short_epochs_writes_both_checkpoints(tmp_path):
    import uaps_amd
    data = uaps_amd.data.SyntheticBatches(2, H=64, W=64, n_batches=2, device=DEV)
    lab = [(xl, yl) for xl, yl, _ in data.items]
    unl = [(xu, yl) for _, yl, xu in data.items]
    tr = _cps_trainer(seed=6)
    hist = tr.fit(lab, unl, lab, epochs=3, iter_per_epoch=3, checkpoint_path=str(tmp_path / "run" / "CPS.pth"))
    assert len(hist) == 2 and tr.iter_num == 4
    for rec in hist:
        for k in ("loss", "cps", "labeled_cps", "val_mdice_1", "val_mdice_2", "val_ce_1", "val_ce_2", "val_loss", "lr_1", "lr_2"):
            assert np.isfinite(rec[k]), k
    assert hist[0]["saved_1"] and hist[0]["saved_2"]            # the first validation beats the initial best of 0
    for which, key in ((1, "best_dice_1"), (2, "best_dice_2")):
        ck = torch.load(str(tmp_path / "run" / f"CPS_{which}.pth"), map_location="cpu", weights_only=True)
        for k in ("epoch", key, "state_dict", "optimizer"):
            assert k in ck, k
        assert ck[key] == tr.best_dice[which - 1]


# ---- 6. what one step launches --------------------------------------------------------------------------------------------------------------

def _kernel_counts(step):
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return {e.key: e.count for e in prof.key_averages()}


def test_one_step_launches_the_cps_kernels_once_and_nothing_for_the_deep_supervision_heads():
    import uaps_amd
    from uaps_amd import conv
    data = uaps_amd.data.SyntheticBatches(2, H=64, W=64, n_batches=1, device=DEV)
    xl, yl, xu = data.items[0]
    tr = _cps_trainer(seed=7)
    counts = _kernel_counts(lambda: tr.train_step(xl, yl, xu))
    assert any("cps_fwd_kernel" in n for n in counts), "the profiler recorded no device kernels of this package"
    assert sum(c for n, c in counts.items() if "cps_fwd_kernel" in n) == 1
    assert sum(c for n, c in counts.items() if "cps_finalize" in n) == 1
    assert sum(c for n, c in counts.items() if "cps_bwd_kernel" in n) == 1
    bad = {n: c for n, c in counts.items()
           if "at::" in n and any(s in n.lower() for s in ("softmax", "argmax", "nll", "catarray", "upsample_nearest"))}
    assert not bad, bad
    # the deep-supervision heads: no gradient, never packed for a convolution kernel, and a step launches every convolution kernel as
    # often as a step of two plain U-Nets (which have no such heads) does
    for m in tr.models:
        for i in (1, 2, 3, 4):
            w = getattr(m.decoder, f"out_conv_dp{i}").weight
            assert w.grad is None and id(w) not in conv._packed
    torch.manual_seed(7)
    plain = uaps_amd.CPSTrainer(uaps_amd.net_factory("unet", 3, 4).to(DEV), uaps_amd.net_factory("unet", 3, 4).to(DEV))
    base = _kernel_counts(lambda: plain.train_step(xl, yl, xu))

    def convs(d):
        return {n: c for n, c in d.items() if "conv" in n.lower()}
    diff = {n: (counts.get(n, 0), base.get(n, 0)) for n in set(counts) | set(base) if counts.get(n, 0) != base.get(n, 0)}
    print("kernels launched a different number of times (UNet_f step, UNet step):", diff)
    assert convs(counts) == convs(base), {n: v for n, v in diff.items() if "conv" in n.lower()}
    # the full 9-tuple forward does launch them: three more convolutions than forward_main
    net = tr.model.eval()
    with torch.no_grad():
        full = _kernel_counts(lambda: net(xl))
        main = _kernel_counts(lambda: net.forward_main(xl))
    assert sum(full.values()) > sum(main.values())
    assert all(id(getattr(net.decoder, f"out_conv_dp{i}").weight) in conv._packed for i in (1, 2, 3))
