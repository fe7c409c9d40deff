"""UCC on the host (no GPU): `cutmix_rects` against the reference's generate_mix_data / generate_crossmix_data (fixture g10_ucc.npz
(c)), `net_factory("unet_ucc")` against the reference's state_dict layout (fixture (a)), the argument checks of the new C entry
points -- each bad call returns before any HIP call, so fake non-null device pointers are never dereferenced -- and of the Python
wrappers, the scalar layout, the trainer's schedule / checkpoint bookkeeping and the hook through which `fit` hands UCCTrainer both
unlabelled views (UCC/UCC_train.py, UCC/cross_cutmix.py)."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from uaps_amd import _lib

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
P = 4096                        # a non-null "device" pointer: the calls below must refuse before touching it
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_ucc.npz")


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def np_cutmix(x_l, y_l, x_wk, x_st, rl, ru):
    """The cut-mix of cross_cutmix.py:78-123 as a plain `where` over the rectangles (flag, y0, y1, x0, x1)."""
    B, _, H, W = x_l.shape
    yy, xx = np.mgrid[0:H, 0:W]

    def inside(r):
        return (r[0] != 0) & (yy >= r[1]) & (yy < r[2]) & (xx >= r[3]) & (xx < r[4])
    out_l, out_y, out_wk, out_st = x_l.copy(), y_l.copy(), x_wk.copy(), x_st.copy()
    for i in range(B):
        m1, m2 = inside(rl[i]), inside(ru[i])
        out_l[i] = np.where(m1, x_l[(i + 1) % B], x_l[i])
        out_y[i] = np.where(m1, y_l[(i + 1) % B], y_l[i])
        out_wk[i] = np.where(m2, out_l[i], x_wk[i])
        out_st[i] = np.where(m2, out_l[i], x_st[i])
    return out_l, out_y, out_wk, out_st


def test_cutmix_rects_reproduce_the_references_mixed_batches():
    from uaps_amd import ucc
    g = np.load(GOLD)
    seed = int(g["mix_seed"])
    B, _, H, W = g["mix_x_l"].shape
    np_rng, py_rng = np.random.RandomState(seed), random.Random(seed)
    rl = ucc.cutmix_rects(B, H, W, np_rng, py_rng, ucc.P_MIX)
    ru = ucc.cutmix_rects(B, H, W, np_rng, py_rng, ucc.P_CROSSMIX)
    assert rl.dtype == np.int32 and rl.shape == ru.shape == (B, 5)
    assert rl[:, 0].tolist() == g["mix_flags"][0].tolist() and ru[:, 0].tolist() == g["mix_flags"][1].tolist()
    for r in (rl, ru):
        assert 0 < r[:, 0].sum() < B                                       # both flags occur in both lists
        assert (r[:, 1] >= 0).all() and (r[:, 2] <= H).all() and (r[:, 3] >= 0).all() and (r[:, 4] <= W).all()
        assert (r[:, 2] > r[:, 1]).all() and (r[:, 4] > r[:, 3]).all()
    out_l, out_y, out_wk, out_st = np_cutmix(g["mix_x_l"], g["mix_y_l"], g["mix_x_wk"], g["mix_x_st"], rl, ru)
    assert np.array_equal(out_l, g["mix_out_l"]) and np.array_equal(out_y, g["mix_out_y"])
    assert np.array_equal(out_wk, g["mix_out_wk"]) and np.array_equal(out_st, g["mix_out_st"])
    assert not np.array_equal(out_l, g["mix_x_l"]) and not np.array_equal(out_wk, g["mix_x_wk"])


def test_unet_ucc_has_the_references_state_dict_and_its_first_perturbation_is_noise():
    import uaps_amd
    from uaps_amd import unet
    g = np.load(GOLD)
    torch.manual_seed(0)
    net = uaps_amd.net_factory("unet_ucc", 3, 4)
    assert isinstance(net, uaps_amd.UNet_UAPS) and net.n_aux == 1 and unet._PERTURBATIONS[0] == "noise"
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]]
    assert {k.split(".")[0] for k in sd} == {"encoder", "main_decoder", "aux_decoder1"}
    assert uaps_amd.net_factory("unet_ucc2", 3, 4) is None


def test_unet_ucc_cpu_main_head_matches_the_reference_fixture():
    import uaps_amd
    from formula_weights import formula_state_dict
    g = np.load(GOLD)
    net = uaps_amd.net_factory("unet_ucc", 3, 4).cpu()
    net.load_state_dict(formula_state_dict(net.state_dict()))
    net.eval()
    with torch.no_grad():
        main = net.forward_main(torch.tensor(g["x"]))
    ref = torch.tensor(g["main_seg"])
    torch.testing.assert_close(main, ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max()))


def test_library_exports_the_ucc_symbols(L):
    for name in ("uaps_ucc_cutmix_batch", "uaps_ucc_cutmix_batch_h", "uaps_ucc_workspace_bytes", "uaps_ucc_fwd", "uaps_ucc_bwd"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None


def _rects(B, H=8, W=8, **edit):
    r = np.zeros((B, 5), dtype=np.int32)
    r[:] = (1, 1, H - 1, 2, W - 2)
    for k, v in edit.items():
        r[0, {"flag": 0, "y0": 1, "y1": 2, "x0": 3, "x1": 4}[k]] = v
    return r


def test_ucc_entry_points_refuse_bad_arguments(L):
    n = C.c_size_t()
    assert L.uaps_ucc_workspace_bytes(2, 4, 8, 8, C.byref(n)) == 0 and n.value > 0
    ws = n.value
    assert L.uaps_ucc_workspace_bytes(2, 4, 8, 8, None) == EINVAL
    assert L.uaps_ucc_workspace_bytes(0, 4, 8, 8, C.byref(n)) == EINVAL
    assert L.uaps_ucc_workspace_bytes(2, 9, 8, 8, C.byref(n)) == ERANGE and L.uaps_ucc_workspace_bytes(2, 1, 8, 8, C.byref(n)) == ERANGE

    def fwd(z1=P, z2=P, y=P, B=2, Cc=4, H=8, W=8, s=P, w=P, wb=None):
        return L.uaps_ucc_fwd(z1, z2, y, B, Cc, H, W, 1e-7, None, None, None, None, s, w, ws if wb is None else wb, None)
    for bad in ({"z1": None}, {"z2": None}, {"y": None}, {"s": None}, {"B": 0}, {"B": -1}, {"H": 0}, {"W": -2}):
        assert fwd(**bad) == EINVAL, bad
    assert fwd(Cc=1) == ERANGE and fwd(Cc=9) == ERANGE
    assert fwd(B=22, Cc=8, H=1024, W=1024) == ERANGE                       # 3 B C H W fp32 = 2.06 GiB
    assert fwd(w=None) == EWORKSPACE and fwd(wb=16) == EWORKSPACE and fwd(wb=ws - 1) == EWORKSPACE

    def bwd(z1=P, z2=P, y=P, s=P, B=2, Cc=4, H=8, W=8, dz1=P, dz2=P):
        return L.uaps_ucc_bwd(z1, z2, y, s, None, None, B, Cc, H, W, dz1, dz2, None)
    for bad in ({"z1": None}, {"z2": None}, {"y": None}, {"s": None}, {"dz1": None}, {"dz2": None}, {"B": 0}, {"H": 0}, {"W": 0}):
        assert bwd(**bad) == EINVAL, bad
    assert bwd(Cc=1) == ERANGE and bwd(Cc=9) == ERANGE
    assert bwd(B=22, Cc=8, H=1024, W=1024) == ERANGE

    keep = []

    def mix(xl=P, xwk=P, xst=P, y=P, rl="ok", ru="ok", B=2, Ci=3, H=8, W=8, out=P, yout=P, hinted=False):
        ptr = []
        for r in (rl, ru):
            if isinstance(r, str):
                r = _rects(max(B, 1), H if H > 2 else 8, W if W > 4 else 8)
            if r is not None:
                keep.append(r)
            ptr.append(None if r is None else r.ctypes.data)
        if hinted:
            return L.uaps_ucc_cutmix_batch_h(None, xl, xwk, xst, y, ptr[0], ptr[1], B, Ci, H, W, out, yout, None)
        return L.uaps_ucc_cutmix_batch(xl, xwk, xst, y, ptr[0], ptr[1], B, Ci, H, W, out, yout, None)
    for hinted in (False, True):
        for bad in ({"xl": None}, {"xwk": None}, {"xst": None}, {"y": None}, {"rl": None}, {"ru": None}, {"out": None}, {"yout": None},
                    {"B": 0}, {"Ci": 0}, {"H": 0}, {"W": -1}):
            assert mix(hinted=hinted, **bad) == EINVAL, bad
        # a rectangle outside the image, or turned inside out -- refused whether or not its flag is set
        for edit in ({"y0": -1}, {"y1": 9}, {"x0": -1}, {"x1": 9}, {"y0": 5, "y1": 4}, {"x0": 7, "x1": 3}, {"flag": 0, "y1": 9}):
            assert mix(hinted=hinted, rl=_rects(2, **edit)) == EINVAL, edit
            assert mix(hinted=hinted, ru=_rects(2, **edit)) == EINVAL, edit
        assert mix(hinted=hinted, B=65) == ERANGE                              # UAPS_UCC_MAX_BATCH
        assert mix(hinted=hinted, B=64, Ci=3, H=2048, W=2048) == ERANGE        # 3 B Cin H W fp32 >= 2 GiB


def test_scalar_layout_of_the_wrapper_is_the_headers():
    from uaps_amd import ucc
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "..", "include", "uaps_hip.h")).read()
    for macro, key in (("UAPS_UCC_S_CE 0", "ce"), ("UAPS_UCC_S_DICE 4", "dice"), ("UAPS_UCC_S_SUP 8", "sup"), ("UAPS_UCC_S_PS 9", "ps"),
                       ("UAPS_UCC_S_PS1 10", "ps_1"), ("UAPS_UCC_S_PS2 11", "ps_2"), ("UAPS_UCC_S_V1 12", "v1"), ("UAPS_UCC_S_E1 13", "e1"),
                       ("UAPS_UCC_S_V2 14", "v2"), ("UAPS_UCC_S_E2 15", "e2"), ("UAPS_UCC_S_BAD 16", "bad")):
        assert "#define " + macro + " " in hdr or "#define " + macro + "\n" in hdr, macro
        assert ucc.s_off(4)[key] == int(macro.split()[-1])
    assert "#define UAPS_UCC_S_NSCALARS(C) (20 + 16 * (C))" in hdr
    assert f"#define UAPS_UCC_MAX_BATCH {ucc.MAX_BATCH}\n" in hdr
    for Cc in (2, 4, 8):
        o = ucc.s_off(Cc)
        assert (o["a1"], o["a2"], o["inter"], o["card"], o["n"]) == (20, 20 + 4 * Cc, 20 + 8 * Cc, 20 + 12 * Cc, 20 + 16 * Cc)
    sc = ucc.ucc_scalars(torch.arange(ucc.s_off(4)["n"], dtype=torch.float32), 4)
    assert sc["ce"].tolist() == [0, 1, 2, 3] and float(sc["ps"]) == 9 and sc["card"].shape == (4, 4)
    assert float(sc["card"][3, 3]) == ucc.s_off(4)["n"] - 1


def test_wrappers_refuse_cpu_tensors_and_bad_rectangles():
    from uaps_amd import ucc
    z = torch.zeros(6, 4, 8, 8)
    with pytest.raises(_lib.UapsHipError):
        ucc.ucc_loss(z, z.clone(), torch.zeros(2, 8, 8, dtype=torch.int64), 2)
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(_lib.UapsHipError):
        ucc.cutmix_batch(x, torch.zeros(2, 8, 8, dtype=torch.int64), x, x, _rects(2), _rects(2))
    assert ucc._check_rects(_rects(2), 2, 8, 8, "r").dtype == np.int32
    for edit in ({"y0": -1}, {"y1": 9}, {"x1": 9}, {"x0": 7, "x1": 3}):
        with pytest.raises(ValueError):
            ucc._check_rects(_rects(2, **edit), 2, 8, 8, "r")
    with pytest.raises(ValueError):
        ucc._check_rects(_rects(3), 2, 8, 8, "r")


def _trainer(seed=1337, **kw):
    import uaps_amd
    torch.manual_seed(3)
    return uaps_amd.UCCTrainer(torch.nn.Conv2d(3, 4, 1), seed=seed, **kw)


def test_schedule_scheduler_and_checkpoint_keys(tmp_path):
    from uaps_amd.ramps import sigmoid_rampup
    tr = _trainer()
    assert tr.ramp_divisor == 150 and tr.rampup == 200
    for it in (0, 149, 150, 12000):
        tr.iter_num = it
        assert tr.consistency_weight() == 0.1 * sigmoid_rampup(it // 150, 200.0), it         # UCC_train.py:244
    assert tr.scheduler.mode == "max" and tr.scheduler.patience == 50 and tr.scheduler.min_lrs == [1e-8]      # :101
    tr.iter_num = 17
    ck = tr.state_for_checkpoint(5, 0.4)
    for key in ("epoch", "best_dice_1", "state_dict", "optimizer", "iter_num", "scheduler", "perturb_rng", "np_global_rng", "cut_np_rng",
                "cut_py_rng"):
        assert key in ck, key
    assert list(ck["state_dict"]) == list(tr.model.state_dict())             # the bare model: no `module.` prefix (:414)
    path = str(tmp_path / "ucc.pth")
    tr.save_checkpoint(path, 5, 0.4)
    assert "best_dice_1" in torch.load(path, weights_only=True)
    want = tr.draw_rects(4, 24, 20)
    other = _trainer(seed=5)
    assert not all(np.array_equal(a, b) for a, b in zip(other.draw_rects(4, 24, 20), want))
    other.load_checkpoint(path)
    assert other.iter_num == 17
    got = other.draw_rects(4, 24, 20)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))                # the next step's rectangles are resumed
    same = _trainer()
    assert all(np.array_equal(a, b) for a, b in zip(same.draw_rects(4, 24, 20), want))     # keyed by (seed, rank)


def test_fit_hands_ucc_both_views_and_leaves_other_trainers_calls_unchanged():
    import uaps_amd
    seen = []

    def stub(self, *args, **kw):
        seen.append((type(self).__name__, args, kw))
        self.iter_num += 1
        return {k: torch.zeros(()) for k in self.log_keys}

    def no_validation(self, batches, pooled=False):
        return {"miou": 0.0, "mdice": 0.5, "acc": 0.0, "ce": 0.0, "loss": 0.0}
    x_l, y_l = torch.full((1, 3, 4, 4), 1.0), torch.zeros(1, 4, 4, dtype=torch.int64)
    wk, st = torch.full((1, 3, 4, 4), 2.0), torch.full((1, 3, 4, 4), 3.0)
    junk = torch.full((1, 4, 4), 9.0)
    ucc_tr = _trainer()
    ucc_tr.train_step, ucc_tr.validate = stub.__get__(ucc_tr), no_validation.__get__(ucc_tr)
    ucc_tr.fit([(x_l, y_l)], [(wk, st, junk, junk)], [], epochs=2, iter_per_epoch=3)
    assert len(seen) == 2
    for name, args, kw in seen:
        assert name == "UCCTrainer" and len(args) == 4 and not kw
        assert torch.equal(args[0], x_l) and torch.equal(args[1], y_l) and torch.equal(args[2], wk) and torch.equal(args[3], st)
    with pytest.raises(ValueError):
        ucc_tr.fit([(x_l, y_l)], [wk], [], epochs=2, iter_per_epoch=2)
    del seen[:]
    torch.manual_seed(3)
    cct = uaps_amd.CCTTrainer(torch.nn.Conv2d(3, 4, 1))
    cct.train_step, cct.validate = stub.__get__(cct), no_validation.__get__(cct)
    cct.fit([(x_l, y_l)], [(wk, junk), st], [], epochs=2, iter_per_epoch=3)      # (x, y) items and bare tensors, as before
    assert [len(a) for _, a, _ in seen] == [3, 3]
    assert torch.equal(seen[0][1][2], wk) and torch.equal(seen[1][1][2], st)
    assert uaps_amd.SegTrainer._unlabeled_inputs(cct, (wk, junk))[0] is wk and uaps_amd.SegTrainer._unlabeled_inputs(cct, st) == (st,)


def test_fixture_stays_within_the_size_limit_for_committed_files():
    assert os.path.getsize(GOLD) <= 1 << 20
