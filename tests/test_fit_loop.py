"""The epoch loop around the step (UAPSTrainer.fit) against the conventions of the reference's Network.run()
(UAPS_train.py:127-159, 279-280, 316-321, 367-402, 427-450; the cycle() form of DAGM-Dataset-codes/UAPS_train.py:143).
The device work (train_step / validate) is scripted here, the loop logic is what is under test; the real thing runs in
tests/test_gpu_trainer.py."""
import os

import numpy as np
import torch

import uaps_amd
from uaps_amd.ramps import get_current_consistency_weight


class _Scripted(uaps_amd.UAPSTrainer):
    def __init__(self, val_dice, **kw):
        net = uaps_amd.UNet_UAPS(3, 4, feature_chns=[2, 2, 2, 2, 2])
        super().__init__(net, loss_fn=lambda *a: None, **kw)
        self.val_dice, self.seen, self.val_calls, self.cw_log = list(val_dice), [], 0, []

    def train_step(self, x_l, y_l, x_u, w=None):
        self.seen.append((float(x_l.flatten()[0]), float(x_u.flatten()[0])))
        self.cw_log.append(self.consistency_weights()[0])
        self.iter_num += 1
        v = torch.tensor(float(self.iter_num))
        return {"loss": v, "sup": v * 2, "unsup": v * 3}

    def epoch_metrics(self, reset=True, pooled=False):
        return {"miou": 0.5, "mdice": 0.25, "acc": 1.0}

    def validate(self, batches, pooled=False):
        d = self.val_dice[self.val_calls]
        self.val_calls += 1
        return {"miou": d / 2, "mdice": d, "acc": 1.0, "ce": 0.1, "dice_loss": 1 - d, "loss": 0.5 * (1 - d + 0.1)}


def _loaders(n_l, n_u):
    lab = [(torch.full((1, 3, 4, 4), float(i)), torch.zeros(1, 4, 4, dtype=torch.long)) for i in range(n_l)]
    unl = [(torch.full((1, 3, 4, 4), 100.0 + i), torch.zeros(1, 4, 4, dtype=torch.long)) for i in range(n_u)]
    return lab, unl


def test_fit_follows_the_reference_loop(tmp_path):
    dice = [0.30, 0.30, 0.45, 0.40]
    tr = _Scripted(dice)
    lab, unl = _loaders(2, 3)
    path = os.path.join(tmp_path, "Checkpoints", "UAPS.pth")
    hist = tr.fit(lab, unl, [None], epochs=5, iter_per_epoch=6, checkpoint_path=path)
    # range(1, epochs) epochs of range(1, iter_per_epoch) steps
    assert [h["epoch"] for h in hist] == [1, 2, 3, 4] and tr.iter_num == 4 * 5
    # a fresh zip(cycle(labelled), cycle(unlabelled)) every epoch: the shorter labelled loader is over-sampled, no StopIteration
    assert tr.seen[:5] == [(0.0, 100.0), (1.0, 101.0), (0.0, 102.0), (1.0, 100.0), (0.0, 101.0)]
    assert tr.seen[5:10] == tr.seen[:5]
    # the logged means divide the running sums by iter_per_epoch, not by the number of steps (:316)
    assert np.isclose(hist[0]["loss"], sum(range(1, 6)) / 6) and np.isclose(hist[1]["unsup"], 3 * sum(range(6, 11)) / 6)
    assert np.isclose(hist[0]["train_mdice"], 0.25 * 5 / 6)
    # strictly greater validation mDice saves (:427), anything else counts patience
    assert [h["saved"] for h in hist] == [True, False, True, False]
    assert [h["patience"] for h in hist] == [0, 1, 0, 1] and hist[-1]["best_dice"] == 0.45
    ck = torch.load(path, weights_only=False)
    assert ck["epoch"] == 3 and ck["best_dice_1"] == 0.45 and ck["iter_num"] == 15
    assert all(k.startswith("module.") for k in ck["state_dict"])
    # scheduler.step(val mDice) once per epoch (:402), mode "max"
    assert tr.scheduler.last_epoch == 4 and np.isclose(tr.scheduler.best, 0.45)


def test_ramp_runs_on_iter_num_across_epochs():
    tr = _Scripted([0.1] * 3, consistency_rampup=4, ramp_divisor=3)
    lab, unl = _loaders(1, 1)
    tr.fit(lab, unl, [None], epochs=4, iter_per_epoch=5)
    want = [get_current_consistency_weight(0.1, i, 4, 3) for i in range(12)]
    assert np.allclose(tr.cw_log, want) and tr.cw_log[0] < tr.cw_log[5] < tr.cw_log[11]


def test_fit_resumes_mid_run(tmp_path):
    dice = [0.2, 0.5, 0.4, 0.6]
    lab, unl = _loaders(2, 2)
    path = os.path.join(tmp_path, "ck.pth")
    full = _Scripted(dice)
    h_full = full.fit(lab, unl, [None], epochs=5, iter_per_epoch=4, checkpoint_path=path + ".full")
    first = _Scripted(dice)
    first.fit(lab, unl, [None], epochs=3, iter_per_epoch=4, checkpoint_path=path)
    ck = torch.load(path, weights_only=False)
    assert ck["epoch"] == 2 and ck["iter_num"] == 6
    second = _Scripted(dice[2:])
    got = second.load_checkpoint(path)
    assert second.iter_num == 6 and second.scheduler.last_epoch == 2
    h2 = second.fit(lab, unl, [None], epochs=5, iter_per_epoch=4, start_epoch=got["epoch"] + 1, best_dice=got["best_dice_1"],
                    checkpoint_path=path)
    assert [h["epoch"] for h in h2] == [3, 4] and second.iter_num == full.iter_num
    assert [h["saved"] for h in h2] == [h["saved"] for h in h_full[2:]] == [False, True]
    assert second.cw_log == full.cw_log[6:]
    # the Dirichlet stream of the mixing weights continues where the checkpoint left it
    assert np.array_equal(second.mix_rng.get_state()[1], first.mix_rng.get_state()[1])


CPS_KEYS = ("loss", "ce_1", "dice_1", "ce_2", "dice_2", "cps", "labeled_cps", "sup", "unsup")


class _ScriptedCPS(uaps_amd.CPSTrainer):
    def __init__(self, dice_1, dice_2, **kw):
        torch.manual_seed(3)
        super().__init__(torch.nn.Conv2d(3, 4, 1), torch.nn.Conv2d(3, 4, 1), **kw)
        self.val_dice, self.val_calls = list(zip(dice_1, dice_2)), 0

    def train_step(self, x_l, y_l, x_u, w=None):
        self.iter_num += 1
        v = torch.tensor(float(self.iter_num))
        res = {k: v * (i + 1) for i, k in enumerate(CPS_KEYS)}
        res.update(cw=self.consistency_weight(), pseudo1=None, pseudo2=None)
        return res

    def epoch_metrics(self, reset=True, pooled=False):
        return {"miou": 0.5, "mdice": 0.25, "acc": 1.0}

    def epoch_metrics2(self, reset=True):
        return {"miou": 0.75, "mdice": 0.125, "acc": 1.0}

    def validate(self, batches, pooled=False):
        d = self.val_dice[self.val_calls]
        self.val_calls += 1
        out = {"loss": 0.5 * (1 - d[0] + 0.1) + 0.5 * (1 - d[1] + 0.2)}
        for s, di, ce in (("_1", d[0], 0.1), ("_2", d[1], 0.2)):
            out.update({"miou" + s: di / 2, "mdice" + s: di, "acc" + s: 1.0, "ce" + s: ce, "dice_loss" + s: 1 - di})
        return out


def test_cps_fit_is_the_same_loop_with_two_networks(tmp_path):
    """CPSTrainer.fit (CPS_train.py:133-512): the record keys, all nine sums over iter_per_epoch, the strict '>' rule and the patience
    count per network, the _1 / _2 files, and a resume through load_checkpoint + best_dice=."""
    d1, d2 = [0.2, 0.5, 0.4, 0.6], [0.3, 0.3, 0.35, 0.1]
    lab, unl = _loaders(2, 3)
    path = os.path.join(tmp_path, "Checkpoints", "CPS.pth")
    full = _ScriptedCPS(d1, d2)
    logged = []
    hist = full.fit(lab, unl, [None], epochs=5, iter_per_epoch=4, checkpoint_path=path, log=logged.append)
    assert logged == hist and [h["epoch"] for h in hist] == [1, 2, 3, 4] and full.iter_num == 4 * 3
    val_keys = {"val_loss"} | {"val_" + k + s for k in ("miou", "mdice", "acc", "ce", "dice_loss") for s in ("_1", "_2")}
    want = {"epoch", "iter_num", "lr_1", "lr_2", "cw", "train_miou_1", "train_mdice_1", "train_miou_2", "train_mdice_2", "saved_1",
            "saved_2", "best_dice_1", "best_dice_2", "patience_1", "patience_2"} | set(CPS_KEYS) | val_keys
    for h in hist:
        assert set(h) == want
    # every one of the nine logged means divides its running sum by iter_per_epoch (:297-308)
    for e, h in enumerate(hist):
        steps = range(3 * e + 1, 3 * e + 4)
        for i, k in enumerate(CPS_KEYS):
            assert np.isclose(h[k], (i + 1) * sum(steps) / 4), (e, k)
        assert h["iter_num"] == 3 * (e + 1) and h["lr_1"] == h["lr_2"] == 1e-3
        assert np.isclose(h["train_mdice_1"], 0.25 * 3 / 4) and np.isclose(h["train_miou_2"], 0.75 * 3 / 4)
        assert np.isclose(h["train_miou_1"], 0.5 * 3 / 4) and np.isclose(h["train_mdice_2"], 0.125 * 3 / 4)
        assert h["val_mdice_1"] == d1[e] and h["val_mdice_2"] == d2[e]
    assert hist[0]["cw"] == get_current_consistency_weight(0.1, 3, 200, 150)
    # per network: strictly greater saves (:457-472), anything else counts patience
    assert [h["saved_1"] for h in hist] == [True, True, False, True] and [h["saved_2"] for h in hist] == [True, False, True, False]
    assert [h["patience_1"] for h in hist] == [0, 0, 1, 0] and [h["patience_2"] for h in hist] == [0, 1, 0, 1]
    assert [h["best_dice_1"] for h in hist] == [0.2, 0.5, 0.5, 0.6] and [h["best_dice_2"] for h in hist] == [0.3, 0.3, 0.35, 0.35]
    assert sorted(os.listdir(os.path.dirname(path))) == ["CPS_1.pth", "CPS_2.pth"]
    p1, p2 = os.path.join(tmp_path, "Checkpoints", "CPS_1.pth"), os.path.join(tmp_path, "Checkpoints", "CPS_2.pth")
    c1, c2 = torch.load(p1, weights_only=True), torch.load(p2, weights_only=True)
    assert c1["epoch"] == 4 and c1["best_dice_1"] == 0.6 and c1["iter_num"] == 12 and c1["patience"] == 0
    assert c2["epoch"] == 3 and c2["best_dice_2"] == 0.35 and c2["iter_num"] == 9 and c2["patience"] == 0
    common = {"epoch", "state_dict", "optimizer", "iter_num", "scheduler", "perturb_rng", "np_global_rng", "patience"}
    assert set(c1) - {"mix_rng"} == common | {"best_dice_1"} and set(c2) - {"mix_rng"} == common | {"best_dice_2"}
    assert list(c1["state_dict"]) == list(full.model.state_dict()) and list(c2["state_dict"]) == list(full.model2.state_dict())
    assert full.scheduler.last_epoch == full.scheduler2.last_epoch == 4
    assert np.isclose(full.scheduler.best, 0.6) and np.isclose(full.scheduler2.best, 0.35)
    # resume after two epochs: network 1's file is of epoch 2, network 2's of epoch 1
    path_r = os.path.join(tmp_path, "resume", "CPS.pth")
    first = _ScriptedCPS(d1, d2)
    first.fit(lab, unl, [None], epochs=3, iter_per_epoch=4, checkpoint_path=path_r)
    second = _ScriptedCPS(d1[2:], d2[2:])
    r1, r2 = second.load_checkpoint(path_r)
    assert (r1["epoch"], r2["epoch"]) == (2, 1) and second.iter_num == 6
    assert second.best_dice == [0.5, 0.3] and second.patience == [0, 0]
    assert second.scheduler.last_epoch == 2 and second.scheduler2.last_epoch == 1
    h2 = second.fit(lab, unl, [None], epochs=5, iter_per_epoch=4, start_epoch=r1["epoch"] + 1,
                    best_dice=(r1["best_dice_1"], r2["best_dice_2"]), checkpoint_path=path_r)
    assert [h["epoch"] for h in h2] == [3, 4] and second.iter_num == full.iter_num
    for k in ("saved_1", "saved_2", "patience_1", "patience_2", "best_dice_1", "best_dice_2", "cw") + CPS_KEYS:
        assert [h[k] for h in h2] == [h[k] for h in hist[2:]], k


class _ScriptedMT(uaps_amd.MeanTeacherTrainer):
    def __init__(self, val_dice, **kw):
        torch.manual_seed(3)
        super().__init__(torch.nn.Conv2d(3, 4, 1), torch.nn.Conv2d(3, 4, 1), **kw)
        self.val_dice, self.val_calls = list(val_dice), 0

    def train_step(self, x_l, y_l, x_u, w=None, teacher_noise=None):
        self.iter_num += 1
        v = torch.tensor(float(self.iter_num))
        return {"loss": v, "sup": v * 2, "unsup": v * 3}

    def epoch_metrics(self, reset=True, pooled=False):
        return {"miou": 0.5, "mdice": 0.25, "acc": 1.0}

    def validate(self, batches, pooled=False):
        d = self.val_dice[self.val_calls]
        self.val_calls += 1
        return {"miou": d / 2, "mdice": d, "acc": 1.0, "ce": 0.1, "dice_loss": 1 - d, "loss": 0.5 * (1 - d + 0.1)}


def test_mean_teacher_fit_logs_one_weight_and_saves_the_teacher(tmp_path):
    tr = _ScriptedMT([0.30, 0.30, 0.45], consistency_rampup=4, ramp_divisor=3)
    lab, unl = _loaders(2, 3)
    path = os.path.join(tmp_path, "MT.pth")
    hist = tr.fit(lab, unl, [None], epochs=4, iter_per_epoch=6, checkpoint_path=path)
    want = {"epoch", "iter_num", "lr", "loss", "sup", "unsup", "train_miou", "train_mdice", "cw1", "cw2", "saved", "best_dice",
            "patience"} | {"val_" + k for k in ("miou", "mdice", "acc", "ce", "dice_loss", "loss")}
    for e, h in enumerate(hist):
        assert set(h) == want
        assert h["cw1"] == get_current_consistency_weight(0.1, 5 * (e + 1), 4, 3) and h["cw2"] == 0.0
        assert np.isclose(h["loss"], sum(range(5 * e + 1, 5 * e + 6)) / 6) and np.isclose(h["train_mdice"], 0.25 * 5 / 6)
    assert hist[-1]["cw1"] == tr.consistency_weight() and hist[0]["cw1"] < hist[-1]["cw1"]
    assert [h["saved"] for h in hist] == [True, False, True] and [h["patience"] for h in hist] == [0, 1, 0]
    assert tr.scheduler.patience == 40 and tr.scheduler.min_lrs == [1e-7] and tr.scheduler.last_epoch == 3
    ck = torch.load(path, weights_only=True)
    assert set(ck) - {"mix_rng"} == {"epoch", "best_dice_1", "state_dict", "optimizer", "iter_num", "scheduler", "ema_state_dict",
                                     "teacher_noise_rng"}
    assert ck["epoch"] == 3 and ck["best_dice_1"] == 0.45 and ck["iter_num"] == 15
    assert list(ck["ema_state_dict"]) == ["module." + k for k in tr.ema_model.state_dict()]
    assert all(torch.equal(ck["ema_state_dict"]["module." + k], v) for k, v in tr.ema_model.state_dict().items())
    other = _ScriptedMT([])
    with torch.no_grad():
        for p in other.ema_model.parameters():
            p.add_(1.0)
    other.noise_rng.offset += 5
    other.load_checkpoint(path)
    assert other.iter_num == 15 and other.scheduler.last_epoch == 3
    assert all(torch.equal(p, q) for p, q in zip(other.ema_model.parameters(), tr.ema_model.parameters()))
    assert (other.noise_rng.seed, other.noise_rng.offset) == (tr.noise_rng.seed, tr.noise_rng.offset)


class _ScriptedBaseline(uaps_amd.BaselineTrainer):
    def __init__(self, val_dice, **kw):
        torch.manual_seed(3)
        super().__init__(torch.nn.Conv2d(3, 4, 1), **kw)
        self.val_dice, self.val_calls, self.unlabelled = list(val_dice), 0, []

    def train_step(self, x_l, y_l, x_u=None, w=None):
        self.unlabelled.append(x_u is not None)
        self.iter_num += 1
        v = torch.tensor(float(self.iter_num))
        return {"loss": v, "ce": v * 2, "dice": v * 3}

    def epoch_metrics(self, reset=True, pooled=False):
        return {"miou": 0.5, "mdice": 0.25, "acc": 1.0}

    def validate(self, batches, pooled=False):
        d = self.val_dice[self.val_calls]
        self.val_calls += 1
        return {"miou": d / 2, "mdice": d, "acc": 1.0, "ce": 0.1, "dice_loss": 1 - d, "loss": 0.5 * (1 - d + 0.1)}


def test_baseline_fit_logs_its_own_scalars_and_no_consistency_weight(tmp_path):
    """BaselineTrainer's step returns loss / ce / dice (baseline_train.py:161-164) and has no consistency term: fit logs those means
    and no cw key; loop, best-checkpoint rule and checkpoint keys are the shared ones."""
    tr = _ScriptedBaseline([0.30, 0.30, 0.45])
    lab, unl = _loaders(2, 3)
    path = os.path.join(tmp_path, "baseline.pth")
    hist = tr.fit(lab, unl, [None], epochs=4, iter_per_epoch=6, checkpoint_path=path)
    want = {"epoch", "iter_num", "lr", "loss", "ce", "dice", "train_miou", "train_mdice", "saved", "best_dice", "patience"} \
        | {"val_" + k for k in ("miou", "mdice", "acc", "ce", "dice_loss", "loss")}
    for e, h in enumerate(hist):
        assert set(h) == want
        s = sum(range(5 * e + 1, 5 * e + 6))
        assert np.isclose(h["loss"], s / 6) and np.isclose(h["ce"], 2 * s / 6) and np.isclose(h["dice"], 3 * s / 6)
        assert np.isclose(h["train_miou"], 0.5 * 5 / 6) and h["lr"] == 1e-3
    assert tr.iter_num == 15 and all(tr.unlabelled)
    assert [h["saved"] for h in hist] == [True, False, True] and [h["patience"] for h in hist] == [0, 1, 0]
    assert tr.scheduler.patience == 40 and tr.scheduler.min_lrs == [1e-7] and tr.scheduler.last_epoch == 3
    ck = torch.load(path, weights_only=True)
    assert set(ck) == {"epoch", "best_dice_1", "state_dict", "optimizer", "iter_num", "scheduler"}
    assert ck["epoch"] == 3 and ck["best_dice_1"] == 0.45 and all(k.startswith("module.") for k in ck["state_dict"])


def test_gradient_destination_is_handed_out_once_per_backward():
    """A parameter used by two autograd nodes of one backward (two forwards of one model: a ragged last batch) must not get
    the same bucket slice twice: the second node would overwrite the first node's gradient and autograd would sum two aliases."""
    from uaps_amd import _graddest
    p = torch.nn.Parameter(torch.zeros(3, 2))
    flat = torch.zeros(8)
    _graddest.register(p, flat, 0)
    try:
        a = _graddest.take(id(p), (3, 2), flat.device)
        b = _graddest.take(id(p), (3, 2), flat.device)
        assert a.data_ptr() == flat.data_ptr() and b.data_ptr() != flat.data_ptr()
        a.fill_(1.0); b.fill_(10.0)
        assert float((a + b).sum()) == 66.0 and float(flat[:6].sum()) == 6.0
        _graddest.new_backward()
        assert _graddest.take(id(p), (3, 2), flat.device).data_ptr() == flat.data_ptr()
        assert _graddest.take(id(p), (2, 3), flat.device).data_ptr() != flat.data_ptr()      # shape mismatch: never the slice
    finally:
        _graddest.unregister(p)
        _graddest.new_backward()
