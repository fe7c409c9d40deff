"""Mean Teacher / UAMT on the GPU: the four kernels of csrc/loss_mean_teacher.hip against float64 restatements of MT/MT_train.py
and UAMT/UA_MT_train.py, the grouped Monte-Carlo teacher forward against the reference's separate forwards, and whole trainer steps
against a float64 oracle built from oracle.uaps_oracle."""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _unet(C=4, seed=0, dropout=False):
    import uaps_amd
    torch.manual_seed(seed)
    m = uaps_amd.UNet(3, C)
    if not dropout:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
    return m


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


# ---- 1. EMA update ----------------------------------------------------------------------------------------------------------------

def _check_ema(ema_before, params, ema_after, step, decay=0.99):
    from uaps_amd.mean_teacher import ema_alpha
    alpha, oma = ema_alpha(decay, step)
    a32, o32 = float(np.float32(alpha)), float(np.float32(oma))
    for e0, p, e1 in zip(ema_before, params, ema_after):
        e0, p, e1 = (t.detach().cpu().numpy() for t in (e0, p, e1))
        if step == 0:
            assert np.array_equal(e1.view(np.uint32), p.view(np.uint32))         # a bit-for-bit copy
            continue
        ref = e0.astype(np.float64) * a32 + o32 * p.astype(np.float64)
        # 1 ulp of the larger of the result and the rounded ema * alpha term (the reference rounds mul_ before add_)
        tol = np.maximum(_ulp(ref), _ulp(e0.astype(np.float64) * a32))
        err = np.abs(e1.astype(np.float64) - ref)
        assert (err <= tol).all(), (step, float((err / tol).max()))


@pytest.mark.parametrize("step", [0, 1, 5, 500])
def test_ema_update_odd_sizes(step):
    from uaps_amd import mean_teacher as mt
    g = torch.Generator().manual_seed(step)
    sizes = [1, 3, 1023, 4097, 5, 70000]
    ema = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, generator=g)) for n in sizes]).to(DEV)
    stu = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, generator=g)) for n in sizes]).to(DEV)
    before = [p.detach().clone() for p in ema]
    mt.ema_update(ema, stu, 0.99, step)
    torch.cuda.synchronize()
    _check_ema(before, list(stu), list(ema), step)


@pytest.mark.parametrize("step", [0, 1, 5, 500])
def test_ema_update_unet_parameters(step):
    from uaps_amd import mean_teacher as mt
    stu, ema = _unet(seed=1).to(DEV), _unet(seed=2).to(DEV)
    bufs = {k: v.clone() for k, v in ema.named_buffers()}
    before = [p.detach().clone() for p in ema.parameters()]
    mt.ema_update(ema, stu, 0.99, step)
    torch.cuda.synchronize()
    _check_ema(before, list(stu.parameters()), list(ema.parameters()), step)
    for k, v in ema.named_buffers():                  # BatchNorm buffers are not averaged (as in the reference)
        assert torch.equal(v, bufs[k]), k


# ---- 2. the teacher's packed weights follow the update -------------------------------------------------------------------------------

def test_teacher_forward_after_ema_update_is_not_stale():
    from uaps_amd import mean_teacher as mt
    stu, ema = _unet(seed=3).to(DEV), _unet(seed=4).to(DEV)
    x = torch.randn(2, 3, 64, 64, device=DEV)
    for train in (False, True):
        ema.train(train)
        with torch.no_grad():
            ema(x)                                    # packs the teacher's weights (and, in train mode, its BatchNorm bounds)
        with torch.no_grad():
            for p in stu.parameters():
                p.add_(torch.randn_like(p) * 0.05)
        mt.ema_update(ema, stu, 0.99, 3)
        fresh = _unet(seed=5).to(DEV)
        fresh.load_state_dict(ema.state_dict())
        fresh.train(train)
        with torch.no_grad():
            got, ref = ema(x), fresh(x)
        assert torch.equal(got, ref), (train, float((got - ref).abs().max()))


# ---- 3. teacher noise ----------------------------------------------------------------------------------------------------------------

def test_teacher_noise_apply_is_bit_identical_to_torch():
    from uaps_amd import mean_teacher as mt
    B, T = 3, 8
    x = torch.randn(B, 3, 40, 36, device=DEV)
    n = torch.randn((1 + T) * B, 3, 40, 36, device=DEV) * 1.5
    got = mt.teacher_inputs(x, T, noise=n)
    ref = x.repeat(1 + T, 1, 1, 1) + torch.clamp(n * 0.1, -0.2, 0.2)     # UA_MT_train.py:181 and :190-194
    assert torch.equal(got, ref)
    x_odd = torch.randn(2, 3, 7, 5, device=DEV)                          # C H W not a multiple of 4: the element-wise form
    n_odd = torch.randn(2, 3, 7, 5, device=DEV)
    assert torch.equal(mt.teacher_inputs(x_odd, 0, noise=n_odd), x_odd + torch.clamp(n_odd * 0.1, -0.2, 0.2))


def test_teacher_noise_distribution_and_streams():
    from uaps_amd import mean_teacher as mt, perturb
    B, T = 16, 8
    x = torch.zeros(B, 3, 256, 256, device=DEV)
    rng = perturb.RngState(1234, mt.NOISE_STREAM)
    a = mt.teacher_inputs(x, T, rng)                  # 9 x 16 x 3 x 256^2 = 2.8e7 draws: the noise itself
    assert a.numel() >= 10 ** 7
    assert float(a.abs().max()) <= float(np.float32(0.2))          # the float32 0.2 of the clamp
    assert abs(float(a.double().mean())) < 1e-3
    clipped = float((a.abs() == 0.2).double().mean())          # P(|N(0,1)| > 2) = 0.0455
    assert abs(clipped - 0.0455) < 0.002, clipped
    assert abs(float(a.double().std()) - 0.0948) < 0.002            # std of clamp(0.1 N, -0.2, 0.2)
    b = mt.teacher_inputs(x, T, perturb.RngState(1234, mt.NOISE_STREAM))
    assert torch.equal(a, b)                                        # same (seed, offset): same noise
    c = mt.teacher_inputs(x, T, rng)                                # the stream moved on
    assert not torch.equal(a, c)
    d = mt.teacher_inputs(x, T, perturb.RngState(perturb._mix(1337, 1), mt.NOISE_STREAM))
    e = mt.teacher_inputs(x, T, perturb.RngState(perturb._mix(1337, 0), mt.NOISE_STREAM))
    assert not torch.equal(d, e)                                    # ranks draw different noise
    # rows are x[r % B] + noise
    x2 = torch.randn(2, 3, 16, 16, device=DEV)
    r = mt.teacher_inputs(x2, 2, perturb.RngState(7, 0)) - x2.repeat(3, 1, 1, 1)
    assert float(r.abs().max()) <= 0.2 + 1e-6           # (x + noise - x: one rounding of the addition)


# ---- 4.-6. fused consistency ---------------------------------------------------------------------------------------------------------

def _ref_uamt(s, e, preds, T, thr, mask_override=None):
    """UA_MT_train.py:194-214 in float64 (preds: raw teacher logits [T*B,C,H,W])."""
    B, C, H, W = s.shape
    p = torch.softmax(preds.double(), dim=1).reshape(T, B, C, H, W).mean(0)
    u = -1.0 * torch.sum(p * torch.log(p + 1e-6), dim=1, keepdim=True)
    m = (u < thr).double()
    if mask_override is not None:
        m = mask_override
    sd = s.double().requires_grad_(True)
    dist = (torch.softmax(sd, 1) - torch.softmax(e.double(), 1)) ** 2
    loss = torch.sum(m * dist) / (2 * torch.sum(m) + 1e-16)
    loss.backward()
    return u, m, loss.detach(), sd.grad


@pytest.mark.parametrize("B,C,H,W", [(2, 2, 64, 64), (4, 2, 64, 64), (2, 4, 64, 64), (4, 4, 64, 64), (2, 7, 64, 64), (4, 7, 64, 64),
                                     (16, 4, 256, 256)])
def test_uamt_consistency_vs_float64(B, C, H, W):
    """Pixels whose float64 uncertainty lies within 1e-4 of the threshold are EXCLUDED from the mask comparison; the reference loss
    and gradient take the kernel's mask decision there (every other pixel's decision must agree)."""
    from uaps_amd import mean_teacher as mt
    T = 8
    g = torch.Generator().manual_seed(B * 100 + C)
    s = torch.randn(B, C, H, W, generator=g) * 2
    e = torch.randn(B, C, H, W, generator=g) * 2
    preds = torch.randn(T * B, C, H, W, generator=g) * 2 + torch.randn(1, C, H, W, generator=g) * 3   # a spread of uncertainties
    p = torch.softmax(preds.double(), 1).reshape(T, B, C, H, W).mean(0)
    u64 = -(p * torch.log(p + 1e-6)).sum(1, keepdim=True)
    thr = float(u64.median())
    sg = s.to(DEV).requires_grad_(True)
    out = mt.mc_consistency_full(sg, e.to(DEV), preds.to(DEV), thr, T=T, want_uncertainty=True)
    out.loss.backward()
    mask = out.mask.cpu().double().unsqueeze(1)
    amb = (u64 - thr).abs() < 1e-4
    u, m_ref, _, _ = _ref_uamt(s, e, preds, T, thr)
    assert torch.equal(mask[~amb], m_ref[~amb])
    _, _, loss, grad = _ref_uamt(s, e, preds, T, thr, mask_override=torch.where(amb, mask, m_ref))
    np.testing.assert_allclose(out.uncertainty.cpu().double().numpy(), u.numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(float(out.loss), float(loss), rtol=1e-5)
    assert float(out.sums[2]) == float(torch.where(amb, mask, m_ref).sum())
    gmax = float(grad.abs().max())
    assert float((sg.grad.cpu().double() - grad).abs().max()) <= 1e-5 * gmax
    # all masked (threshold below every u): loss 0 and gradient 0 through the 1e-16 guard
    sg2 = s.to(DEV).requires_grad_(True)
    l0 = mt.mc_consistency(sg2, e.to(DEV), preds.to(DEV), -1.0, T=T)
    l0.backward()
    assert float(l0) == 0.0 and float(sg2.grad.abs().max()) == 0.0
    # nothing masked: the plain sum over all pixels / (2 B H W)
    sg3 = s.to(DEV).requires_grad_(True)
    l1 = mt.mc_consistency(sg3, e.to(DEV), preds.to(DEV), 100.0, T=T)
    l1.backward()
    _, _, loss1, grad1 = _ref_uamt(s, e, preds, T, 100.0)
    np.testing.assert_allclose(float(l1), float(loss1), rtol=1e-5)
    assert float((sg3.grad.cpu().double() - grad1).abs().max()) <= 1e-5 * float(grad1.abs().max())


@pytest.mark.parametrize("C", [2, 4])
def test_probability_form_against_fixture_g8(golden_dir, C):
    """The call form of sibling.uamt_consistency_loss (averaged probabilities, T = 0) against the recorded reference values."""
    import os
    from uaps_amd import mean_teacher as mt
    g = np.load(os.path.join(golden_dir, "g8_sibling.npz"))
    student = torch.tensor(g[f"uamt{C}_student"], device=DEV, requires_grad=True)
    ema, preds = torch.tensor(g[f"uamt{C}_ema"], device=DEV), torch.tensor(g[f"uamt{C}_preds"], device=DEV)
    loss = mt.mc_consistency(student, ema, preds, float(g[f"uamt{C}_threshold"]))
    loss.backward()
    np.testing.assert_allclose(float(loss), float(g[f"uamt{C}_loss"]), rtol=2e-5)
    ref = g[f"uamt{C}_dstudent"]
    np.testing.assert_allclose(student.grad.cpu().numpy(), ref, rtol=2e-3, atol=2e-5 * float(np.abs(ref).max()))


@pytest.mark.parametrize("B,C,H,W", [(2, 4, 64, 64), (3, 7, 33, 45), (16, 4, 256, 256)])
def test_mt_consistency_vs_float64(B, C, H, W):
    from uaps_amd import mean_teacher as mt
    g = torch.Generator().manual_seed(C * 7 + B)
    s, e = torch.randn(B, C, H, W, generator=g) * 2, torch.randn(B, C, H, W, generator=g) * 2
    sd = s.double().requires_grad_(True)
    ref = torch.mean((torch.softmax(sd, 1) - torch.softmax(e.double(), 1)) ** 2)        # MT_train.py:199
    (ref * 0.37).backward()
    sg = s.to(DEV).requires_grad_(True)
    loss = mt.mc_consistency(sg, e.to(DEV))
    (loss * 0.37).backward()
    np.testing.assert_allclose(float(loss), float(ref), rtol=1e-5)
    assert float((sg.grad.cpu().double() - sd.grad).abs().max()) <= 1e-5 * float(sd.grad.abs().max())


# ---- 7. grouped Monte-Carlo teacher forward -------------------------------------------------------------------------------------------

def test_grouped_mc_forward_matches_separate_forwards():
    """ONE forward of 8B images under stat_groups(4) against four forwards of 2B (UA_MT_train.py:188-196), train mode, dropout off.
    Tolerance: the grouped and the separate forwards run the same kernels, but the BatchNorm partial sums are taken about the running
    mean as it stands when the layer runs (_STAT_SHIFT), which differs between one and four successive forwards -- another fp32
    rounding of the same statistics: logits within 2e-4 of their max magnitude, running statistics within rtol 1e-5 / atol 1e-6."""
    from uaps_amd import fused
    B = 2
    net = _unet(seed=11).to(DEV).train()
    sep = copy.deepcopy(net)
    x = torch.randn(8 * B, 3, 64, 64, device=DEV)
    with torch.no_grad():
        with fused.stat_groups(4):
            got = net(x)
        ref = torch.cat([sep(x[2 * B * i:2 * B * (i + 1)]) for i in range(4)])
    scale = float(ref.abs().max())
    assert float((got - ref).abs().max()) <= 2e-4 * scale
    for (k, a), (_, b) in zip(net.named_buffers(), sep.named_buffers()):
        if a.is_floating_point():
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6, msg=k)
        else:
            assert torch.equal(a, b), k


# ---- 8.-9. trainer steps against a float64 oracle -------------------------------------------------------------------------------------

def _sd64(model, grad):
    sd = {k: (v.detach().cpu().clone().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    if grad:
        for k in sd:
            if k.endswith(".weight") or k.endswith(".bias"):
                sd[k].requires_grad_(True)
    return sd


def _fwd(x, sd):
    from oracle import uaps_oracle as O
    return O.decoder_forward(O.encoder_forward(x, sd, "encoder", True, dropout=[0.0] * 5), sd, "decoder", True)


def _models(C=4):
    stu = _unet(C, seed=31)
    ema = _unet(C, seed=32)
    with torch.no_grad():        # confident logits: the entropy mask keeps some pixels and drops others
        for m in (stu, ema):
            m.decoder.out_conv.weight.mul_(8.0)
    return stu, ema


def _oracle_step(stu, ema, x_l, y_l, x_u, noise, iter_num, uamt, T=8):
    """One step of UA_MT_train.py:174-233 (uamt) or MT_train.py:175-219 in float64 on the CPU.  Returns the scalars, the student
    gradients, the student after Adam and the alpha of the EMA, plus the bounds of the consistency term when the float64 mask has
    pixels within 1e-4 of the threshold (the kernel's float32 decision may go either way there)."""
    from oracle import uaps_oracle as O
    from uaps_amd import sibling
    from uaps_amd.ramps import get_current_consistency_weight
    B = x_l.shape[0]
    sd, te = _sd64(stu, True), _sd64(ema, False)
    lab, un = _fwd(x_l.double(), sd), _fwd(x_u.double(), sd)
    inputs = (x_u.repeat(1 + (T if uamt else 0), 1, 1, 1) + torch.clamp(noise * 0.1, -0.2, 0.2)).double()
    with torch.no_grad():
        e = _fwd(inputs[:B], te)
    ce, dice = O.cross_entropy(lab, y_l), O.dice_loss(y_l.unsqueeze(1), lab)
    sup = 0.5 * (dice + ce)
    dist = (torch.softmax(un, 1) - torch.softmax(e, 1)) ** 2
    out = {"ce": ce, "dice": dice}
    if uamt:
        cw = get_current_consistency_weight(0.1, iter_num, 200, 80)
        with torch.no_grad():
            preds = torch.cat([_fwd(inputs[B + 2 * B * i:B + 2 * B * (i + 1)], te) for i in range(T // 2)])
            p = torch.softmax(preds, 1).reshape(T, B, *preds.shape[1:]).mean(0)
            u = -1.0 * torch.sum(p * torch.log(p + 1e-6), dim=1, keepdim=True)
        thr = sibling.uamt_threshold(cw)
        mask = (u < thr).double()
        amb = ((u - thr).abs() < 1e-4).double()
        cons = torch.sum(mask * dist) / (2 * torch.sum(mask) + 1e-16)
        with torch.no_grad():
            lo_m, hi_m = mask * (1 - amb), torch.clamp(mask + amb, max=1)
            out["cons_range"] = sorted(float(torch.sum(m * dist) / (2 * torch.sum(m) + 1e-16)) for m in (lo_m, hi_m))
        out["mask_frac"] = float(mask.mean())
        wc = cw
    else:
        cw = get_current_consistency_weight(0.1, iter_num, 200, 150)
        cons = torch.mean(dist)
        wc = cw if iter_num >= 1000 else 0.0
        out["cons_range"] = [float(cons)] * 2 if iter_num >= 1000 else [0.0, 0.0]
    loss = sup + wc * cons
    loss.backward()
    pkeys = [k for k in sd if sd[k].requires_grad]
    grads = {k: sd[k].grad.clone() for k in pkeys}
    opt = torch.optim.Adam([sd[k] for k in pkeys], lr=1e-3)
    opt.step()
    out.update(loss=float(loss), cw=cw, wc=wc, grads=grads, new={k: sd[k].detach() for k in pkeys},
               alpha=min(1 - 1 / (iter_num + 1), 0.99))
    return out


def _run_and_compare(uamt, iter_num):
    import uaps_amd
    rng = np.random.default_rng(5 + iter_num)
    B, C, H, W, T = 4, 4, 64, 64, 8
    stu, ema = _models(C)
    x_l = torch.tensor(rng.standard_normal((B, 3, H, W)).astype(np.float32))
    x_u = torch.tensor(rng.standard_normal((B, 3, H, W)).astype(np.float32))
    y_l = torch.tensor(uaps_amd.data.synthetic_masks(rng, B, C, H, W))
    noise = torch.tensor(rng.standard_normal(((1 + (T if uamt else 0)) * B, 3, H, W)).astype(np.float32))
    ref = _oracle_step(stu, ema, x_l, y_l, x_u, noise, iter_num, uamt, T)
    init = {k: v.detach().clone() for k, v in stu.named_parameters()}
    ema_init = {k: v.detach().clone().double() for k, v in ema.named_parameters()}
    stu.to(DEV)
    ema.to(DEV)
    cls = uaps_amd.UAMTTrainer if uamt else uaps_amd.MeanTeacherTrainer
    tr = cls(stu, ema, base_lr=1e-3)
    tr.iter_num = iter_num
    captured = {}
    hooks = [p.register_hook(lambda g, n=n: captured.__setitem__(n, g.detach().clone())) for n, p in stu.named_parameters()]
    res = tr.train_step(x_l.to(DEV), y_l.to(DEV), x_u.to(DEV), teacher_noise=noise.to(DEV))
    for h in hooks:
        h.remove()
    assert res["cw"] == ref["cw"]
    np.testing.assert_allclose(float(res["ce"]), float(ref["ce"]), rtol=2e-5)
    np.testing.assert_allclose(float(res["dice"]), float(ref["dice"]), rtol=2e-5)
    lo, hi = ref["cons_range"]
    cons = float(res["consistency"])
    assert lo * (1 - 2e-5) - 1e-9 <= cons <= hi * (1 + 2e-5) + 1e-9, (cons, lo, hi)
    np.testing.assert_allclose(float(res["loss"]), ref["loss"], rtol=2e-5, atol=ref["wc"] * (hi - lo) + 1e-9)
    lr, checked = 1e-3, 0
    for n, p in stu.named_parameters():
        g_ref = ref["grads"][n]
        scale = float(g_ref.abs().max())
        err = float((captured[n].cpu().double() - g_ref).abs().max())
        assert err <= max(5e-3 * scale, 1e-5), f"{n}: max err {err:.3e} vs scale {scale:.3e}"       # as test_gpu_trainer's baseline step
        sure = g_ref.abs() > max(1e-5, 1e-2 * scale)
        delta, delta_ref = p.detach().cpu() - init[n], (ref["new"][n] - init[n].double()).float()
        checked += int(sure.sum())
        if sure.any():
            assert float((delta[sure] - delta_ref[sure]).abs().max()) <= 0.02 * lr, n
    assert checked > 10000
    # the teacher after the EMA: alpha * teacher + (1 - alpha) * (the student after THIS step's Adam)
    a = ref["alpha"]
    for n, p in ema.named_parameters():
        want = ema_init[n] * np.float32(a) + np.float32(1 - a) * stu.get_parameter(n).detach().cpu().double()
        assert float((p.detach().cpu().double() - want).abs().max()) <= 2 * float(_ulp(want.numpy()).max()), n
    return res, ref


@pytest.mark.parametrize("iter_num", [0, 12000])
def test_uamt_step_vs_float64_oracle(iter_num):
    res, ref = _run_and_compare(True, iter_num)
    assert res["cw"] > 0 and res["threshold"] == pytest.approx((0.75 + 2.5 * res["cw"]) * math.log(2))
    assert 0.05 < ref["mask_frac"] < 0.95, ref["mask_frac"]          # the mask is neither empty nor full: the gradient is exercised
    assert float(res["consistency"]) > 0


def test_mt_step_before_the_gate_has_no_consistency_gradient():
    res, ref = _run_and_compare(False, 999)
    assert float(res["consistency"]) == 0.0 and float(res["loss"]) == float(res["sup"])


def test_mt_step_after_the_gate_vs_float64_oracle():
    res, ref = _run_and_compare(False, 1000)
    assert ref["wc"] > 0 and float(res["consistency"]) > 0


# ---- 10. checkpoints and the epoch loop ------------------------------------------------------------------------------------------------

def test_checkpoint_round_trip_resumes_bit_identically(tmp_path):
    import uaps_amd
    B, T = 2, 8
    data = uaps_amd.data.SyntheticBatches(B, H=64, W=64, n_batches=2, device=DEV)
    g = torch.Generator().manual_seed(3)
    noises = [torch.randn((1 + T) * B, 3, 64, 64, generator=g).to(DEV) for _ in range(2)]

    def trainer():
        stu, ema = _models()
        return uaps_amd.UAMTTrainer(stu.to(DEV), ema.to(DEV))
    a = trainer()
    a.train_step(*data.items[0], teacher_noise=noises[0])
    path = str(tmp_path / "uamt.pth")
    a.save_checkpoint(path, 1, 0.5)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    for k in ("epoch", "best_dice_1", "state_dict", "optimizer", "ema_state_dict"):
        assert k in ck, k
    ra = a.train_step(*data.items[1], teacher_noise=noises[1])
    b = trainer()
    b.load_checkpoint(path)
    rb = b.train_step(*data.items[1], teacher_noise=noises[1])
    for k in ("loss", "ce", "dice", "consistency"):
        assert torch.equal(ra[k], rb[k]), k
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), n
    for (n, p), (_, q) in zip(a.ema_model.state_dict().items(), b.ema_model.state_dict().items()):
        assert torch.equal(p, q), n
    # a reference checkpoint (student only) leaves the teacher as it is
    ref_ck = {k: ck[k] for k in ("epoch", "best_dice_1", "state_dict", "optimizer")}
    torch.save(ref_ck, path)
    before = {k: v.clone() for k, v in b.ema_model.state_dict().items()}
    b.load_checkpoint(path)
    for k, v in b.ema_model.state_dict().items():
        assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("cls", ["MeanTeacherTrainer", "UAMTTrainer"])
def test_fit_two_short_epochs_with_validation(cls):
    import uaps_amd
    data = uaps_amd.data.SyntheticBatches(2, H=64, W=64, n_batches=2, device=DEV)
    lab = [(xl, yl) for xl, yl, _ in data.items]
    unl = [(xu, yl) for _, yl, xu in data.items]
    stu, ema = _unet(seed=41, dropout=True), _unet(seed=42, dropout=True)
    tr = getattr(uaps_amd, cls)(stu.to(DEV), ema.to(DEV))
    hist = tr.fit(lab, unl, lab, epochs=3, iter_per_epoch=3)
    assert len(hist) == 2 and tr.iter_num == 4
    for rec in hist:
        assert np.isfinite(rec["loss"]) and np.isfinite(rec["val_mdice"]) and np.isfinite(rec["val_ce"])
