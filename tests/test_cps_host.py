"""CPS on the host (no GPU): the new symbols and the argument checks of the C entry points -- each bad call returns before any HIP call,
so fake non-null device pointers are never dereferenced -- the UNet_f network against the reference's state_dict layout (fixture
g9_cps.npz), the consistency ramp, and the per-network scheduler / best-checkpoint / checkpoint bookkeeping of CPSTrainer
(CPS/CPS_train.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from uaps_amd import _lib

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
P = 4096                        # a non-null "device" pointer: the calls below must refuse before touching it
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_cps.npz")


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_library_exports_the_cps_symbols(L):
    for name in ("uaps_cps_workspace_bytes", "uaps_cps_fwd", "uaps_cps_bwd"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None


def _ws(L, N=4, B_lab=2, Cc=4, H=8, W=8):
    n = C.c_size_t()
    assert L.uaps_cps_workspace_bytes(N, B_lab, Cc, H, W, C.byref(n)) == 0 and n.value > 0
    return n.value


def test_cps_entry_points_refuse_bad_arguments(L):
    ws = _ws(L)
    assert L.uaps_cps_workspace_bytes(4, 2, 4, 8, 8, None) == EINVAL
    n = C.c_size_t()
    assert L.uaps_cps_workspace_bytes(4, 5, 4, 8, 8, C.byref(n)) == EINVAL
    assert L.uaps_cps_workspace_bytes(4, 2, 9, 8, 8, C.byref(n)) == ERANGE

    def fwd(z1=P, z2=P, y=P, N=4, B_lab=2, Cc=4, H=8, W=8, p1=None, p2=None, s=P, w=P, wb=None):
        return L.uaps_cps_fwd(z1, z2, y, N, B_lab, Cc, H, W, 1e-7, p1, p2, s, w, ws if wb is None else wb, None)
    for bad in ({"z1": None}, {"z2": None}, {"y": None}, {"s": None}, {"N": 0}, {"H": 0}, {"W": -2},
                {"B_lab": 5}, {"B_lab": 4}, {"B_lab": 0}, {"B_lab": -1}):      # B_lab > N; no unlabelled / no labelled rows
        assert fwd(**bad) == EINVAL, bad
    assert fwd(Cc=1) == ERANGE and fwd(Cc=9) == ERANGE
    assert fwd(N=64, B_lab=32, Cc=8, H=1024, W=1024) == ERANGE                # 2 GiB of fp32
    assert fwd(w=None) == EWORKSPACE and fwd(wb=16) == EWORKSPACE and fwd(wb=ws - 1) == EWORKSPACE

    def bwd(z1=P, z2=P, y=P, s=P, N=4, B_lab=2, Cc=4, H=8, W=8, dz1=P, dz2=P):
        return L.uaps_cps_bwd(z1, z2, y, s, None, None, None, N, B_lab, Cc, H, W, dz1, dz2, None)
    for bad in ({"z1": None}, {"z2": None}, {"y": None}, {"s": None}, {"dz1": None}, {"dz2": None}, {"N": -1}, {"H": 0}, {"W": 0},
                {"B_lab": 5}, {"B_lab": 4}, {"B_lab": 0}):
        assert bwd(**bad) == EINVAL, bad
    assert bwd(Cc=1) == ERANGE and bwd(Cc=9) == ERANGE
    assert bwd(N=64, B_lab=32, Cc=8, H=1024, W=1024) == ERANGE


def test_scalar_layout_of_the_wrapper_is_the_headers():
    from uaps_amd import cps
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "..", "include", "uaps_hip.h")).read()
    for macro, key in (("UAPS_CPS_S_CE 0", "ce"), ("UAPS_CPS_S_DICE 6", "dice"), ("UAPS_CPS_S_SUP 12", "sup"),
                       ("UAPS_CPS_S_LCPS 13", "labeled_cps"), ("UAPS_CPS_S_CPS 14", "cps"), ("UAPS_CPS_S_BAD 15", "bad")):
        assert "#define " + macro in hdr, macro
        assert cps.s_off(4)[key] == int(macro.split()[-1])
    assert "#define UAPS_CPS_S_NSCALARS(C) (16 + 24 * (C))" in hdr
    for Cc in (2, 4, 8):
        o = cps.s_off(Cc)
        assert (o["a1"], o["a2"], o["inter"], o["card"], o["n"]) == (16, 16 + 6 * Cc, 16 + 12 * Cc, 16 + 18 * Cc, 16 + 24 * Cc)
    sc = cps.cps_scalars(torch.arange(cps.s_off(4)["n"], dtype=torch.float32), 4)
    assert sc["ce"].tolist() == [0, 1, 2, 3, 4, 5] and float(sc["cps"]) == 14 and sc["card"].shape == (6, 4)
    assert float(sc["card"][5, 3]) == cps.s_off(4)["n"] - 1


def test_unet_f_has_the_references_state_dict_and_loads_it_strictly():
    import uaps_amd
    from uaps_amd.unet import UNet_f
    g = np.load(GOLD)
    torch.manual_seed(0)
    net = uaps_amd.net_factory("unet_f", 3, 4)
    assert isinstance(net, UNet_f) and isinstance(net, uaps_amd.UNet)
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]]
    for i in (1, 2, 3, 4):
        assert f"decoder.out_conv_dp{i}.weight" in sd
    ref_shaped = {str(k): torch.zeros(eval(str(s))) if "num_batches" not in str(k) else torch.zeros((), dtype=torch.int64)
                  for k, s in zip(g["keys"], g["shapes"])}
    net.load_state_dict(ref_shaped, strict=True)
    assert float(net.decoder.out_conv_dp4.weight.abs().max()) == 0.0


def test_unet_f_cpu_forward_is_the_references_nine_tuple():
    """The CPU path (plain torch modules) against fixture (b); the GPU test checks the HIP path against the same numbers."""
    import uaps_amd
    from formula_weights import formula_state_dict
    g = np.load(GOLD)
    net = uaps_amd.net_factory("unet_f", 3, 4).cpu()
    net.load_state_dict(formula_state_dict(net.state_dict()))
    net.eval()
    x = torch.tensor(g["x"])
    with torch.no_grad():
        out = net(x)
        main = net.forward_main(x)
    assert len(out) == 9 and out[0].shape == (1, 256, 2, 2) and out[4].shape == (1, 16, 32, 32)
    for i in range(4):
        ref = torch.tensor(g[f"dp{i}"])
        assert out[5 + i].shape == ref.shape == (1, 4, 32, 32)
        torch.testing.assert_close(out[5 + i], ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max()))
    assert torch.equal(main, out[5])


def _trainer(seed=1337, **kw):
    import uaps_amd
    torch.manual_seed(3)
    return uaps_amd.CPSTrainer(torch.nn.Conv2d(3, 4, 1), torch.nn.Conv2d(3, 4, 1), seed=seed, **kw)


def test_cw_is_a_tenth_of_the_sigmoid_ramp_on_iter_over_150():
    from uaps_amd.ramps import sigmoid_rampup
    tr = _trainer()
    assert tr.ramp_divisor == 150 and tr.rampup == 200
    for it in (0, 1, 149, 150, 151, 5 * 150 + 3, 12000, 300 * 150):
        tr.iter_num = it
        assert tr.consistency_weight() == 0.1 * sigmoid_rampup(it // 150, 200.0), it          # CPS_train.py:247
    tr.iter_num = 0
    assert tr.consistency_weight() > 0


def test_two_optimizers_two_schedulers_and_two_best_checkpoint_rules():
    """CPS_train.py:115-119, :414-415, :457-472, in the manner of tests/test_fit_loop.py: per network, strict '>' against the best."""
    tr = _trainer(base_lr=1e-3)
    assert tr.optimizer is not tr.optimizer2 and tr.scheduler is not tr.scheduler2
    assert [id(p) for p in tr.optimizer.param_groups[0]["params"]] == [id(p) for p in tr.model.parameters()]
    assert [id(p) for p in tr.optimizer2.param_groups[0]["params"]] == [id(p) for p in tr.model2.parameters()]
    for s in (tr.scheduler, tr.scheduler2):
        assert s.mode == "max" and s.patience == 50 and s.min_lrs == [1e-7]
    assert tr.note_validation(0.30, 0.20) == (True, True)
    assert tr.note_validation(0.30, 0.25) == (False, True)                  # equal is not better (:457)
    assert tr.note_validation(0.10, 0.25) == (False, False)
    assert tr.best_dice == [0.30, 0.25] and tr.patience == [2, 1]
    # network 1 stalls for more than `patience` validations while network 2 keeps improving: only lr_1 drops
    for i in range(52):
        tr.note_validation(0.10, 0.26 + 1e-3 * i)
    lr1, lr2 = tr.learning_rates()
    assert lr1 == pytest.approx(1e-4) and lr2 == pytest.approx(1e-3)


def test_checkpoints_hold_the_references_keys_per_network(tmp_path):
    from uaps_amd import cps
    tr = _trainer()
    tr.note_validation(0.4, 0.6)
    tr.iter_num = 17
    c1, c2 = tr.state_for_checkpoint(5, which=1), tr.state_for_checkpoint(5, which=2)
    for key in ("epoch", "state_dict", "optimizer", "iter_num", "scheduler", "perturb_rng", "np_global_rng", "patience"):
        assert key in c1 and key in c2, key
    assert c1["best_dice_1"] == 0.4 and "best_dice_2" not in c1
    assert c2["best_dice_2"] == 0.6 and "best_dice_1" not in c2
    assert list(c1["state_dict"]) == list(tr.model.state_dict())            # CPS saves the bare model: no `module.` prefix (:483)
    assert all(torch.equal(c2["state_dict"][k], v) for k, v in tr.model2.state_dict().items())
    assert cps.checkpoint_paths("a/b.pth") == ("a/b_1.pth", "a/b_2.pth") and cps.checkpoint_paths(("x", "y")) == ("x", "y")
    path = str(tmp_path / "cps.pth")
    tr.save_checkpoint(path, 5)
    assert sorted(os.listdir(tmp_path)) == ["cps_1.pth", "cps_2.pth"]
    assert "best_dice_2" in torch.load(str(tmp_path / "cps_2.pth"), weights_only=True)
    other = _trainer(seed=5)
    with torch.no_grad():
        for p in list(other.model.parameters()) + list(other.model2.parameters()):
            p.add_(1.0)
    other.load_checkpoint(path)
    assert other.iter_num == 17 and other.best_dice == [0.4, 0.6]
    for a, b in ((tr.model, other.model), (tr.model2, other.model2)):
        assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))


def test_cps_trainer_refuses_one_module_twice_and_more_than_one_rank(monkeypatch):
    import uaps_amd
    from uaps_amd import dist
    m = torch.nn.Conv2d(3, 4, 1)
    with pytest.raises(ValueError):
        uaps_amd.CPSTrainer(m, m)
    monkeypatch.setattr(dist, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError):
        uaps_amd.CPSTrainer(m, torch.nn.Conv2d(3, 4, 1))


def test_cps_loss_refuses_cpu_tensors_and_bad_shapes():
    from uaps_amd import cps
    z = torch.zeros(4, 4, 8, 8)
    with pytest.raises(_lib.UapsHipError):
        cps.cps_loss(z, z.clone(), torch.zeros(2, 8, 8, dtype=torch.int64), 2)
