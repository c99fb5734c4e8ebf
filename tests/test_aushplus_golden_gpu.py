"""GPU tests of AushPlus against the reference's own recorded runs (tests/golden/aushplus_*.npz, written by
tests/golden/make_golden_aushplus.py with the same numpy / torch seeds the tests set).

  from init (aushplus_game_init): the template forward, the first pretrain_G batch (loss, gradient fingerprints) and the first
      train_D batch (loss) with the single-step tolerances of tests/test_aushplus_gpu.py (A_TOL 1e-5; class / value exactly,
      the recorded margin is 0.35; losses 1e-5 relative; gradient fingerprints 2e-4 / 1e-4 as in test_aushplus_golden_host.py).
  small-case trajectory (aushplus_small): a whole train_step on 60 users.  The fixture's run-minimum of min_k |a - b_k| over
      every consumed entry is 2.0e-3 (>= 20 A_TOL); the device's own run-minimum must be above half of it before anything else
      is compared.  Then the classes cannot differ, so value, class and generate_fake's non-zeros are compared exactly, the final
      a within half the recorded run-minimum (what keeps the classes), and the phase losses within 1e-4 relative (about ten
      dependent Adam steps of single-step error 1e-5).
  game-sized short step (aushplus_game_step): per quantity within 3 x the recorded |float32 - float64| difference of the
      reference itself (floor: the single-step tolerance), and at most 1 % of the template entries in another class than the
      float32 reference at the end of the step."""
import os

import numpy as np
import pytest
import torch

from recad_amd import dataset, model

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G_NAMES = ("min_boundary_value", "interval_lengths", "layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias")
D_NAMES = ("main.0.weight", "main.0.bias", "main.2.weight", "main.2.bias", "main.4.weight", "main.4.bias")
A_TOL = 1e-5
PHASES = {"pretrain_G": "pretrain_g", "train_D": None, "train_G_adv": "gan_g", "train_G_attack": "attack"}


def _fp(a):
    a = np.asarray(a, dtype=np.float64)
    return np.asarray([a.sum(), (a * a).sum()])


def _game(dev):
    g = np.load(os.path.join(GOLDEN, "aush_game_partial.npz"))
    full = dataset.from_config("explicit", "game", device=dev, train_dict=g["train_kvr"], valid_dict=g["valid_kvr"],
                               test_dict=g["test_kvr"])
    np.random.seed(int(g["seed"]))
    return full.partial_sample(user_ratio=float(g["user_ratio"]))


class _DenseData:
    def __init__(self, mat):
        self.mat = mat

    def info_describe(self):
        return {"n_users": self.mat.shape[0], "n_items": self.mat.shape[1], "train_mat": self.mat}


def _build(g, ds, dev):
    cfg = {k[4:]: g[k].item() for k in g.files if k.startswith("cfg_")}
    np.random.seed(int(g["seed"]))
    torch.manual_seed(int(g["seed"]))
    att = model.from_config("attacker", "aushplus", device=dev, **cfg).I(dataset=ds)
    assert np.array_equal(att.template_users, g["template_users"]) and np.array_equal(att.template_cols, g["pos_cols"])
    return att


def _device_losses(att):
    """The phase values in the fixture's order.  The fixture holds what the reference's train_G returns third, the ATTACK loss,
    which is 0.0 for the adversarial call; the device's adversarial BCE has no recorded counterpart and is only checked finite."""
    ph = att.last_phase_losses
    assert np.isfinite(ph["gan_g"]).all()
    return np.asarray(ph["pretrain_g"] + ph["pretrain_d"] + ph["gan_d"] + [0.0] * len(ph["gan_g"]) + ph["attack"])


def test_from_init_against_the_reference(gpu_device):
    g = np.load(os.path.join(GOLDEN, "aushplus_game_init.npz"))
    att = _build(g, _game(gpu_device), gpu_device)
    out = att.last_forward()
    print(f"from init: max |a_dev - a_ref| {np.abs(out['a'] - g['a']).max():.2e}")
    assert np.abs(out["a"] - g["a"]).max() <= A_TOL
    assert np.array_equal(out["cls"], g["cls"]) and np.array_equal(out["value"], g["value"])
    loss = att.pretrain_G(perm=g["pretrain_users"])
    print(f"first pretrain_G batch: device {loss:.8f} reference {float(g['pretrain_loss']):.8f}")
    assert abs(loss - float(g["pretrain_loss"])) <= 1e-5 * float(g["pretrain_loss"])
    grads = att.generator_grad()
    for k, want, amax in zip(G_NAMES, g["pretrain_grad_fp"], g["pretrain_grad_absmax"]):
        got = grads[k].numpy().astype(np.float64)
        assert abs((got * got).sum() - want[1]) <= 2e-4 * want[1], k
        assert abs(got.sum() - want[0]) <= 1e-4 * np.abs(got).sum(), k
        assert abs(np.abs(got).max() - amax) <= 1e-4 * amax, k
    d_loss = att.train_D(perm=g["d_users"])
    print(f"first train_D batch: device {d_loss:.8f} reference {float(g['d_loss']):.8f}")
    assert abs(d_loss - float(g["d_loss"])) <= 1e-5 * float(g["d_loss"])


def test_small_case_trajectory_against_the_reference(gpu_device):
    g = np.load(os.path.join(GOLDEN, "aushplus_small.npz"))
    ptr, idx, val = g["small_ptr"], g["small_idx"], g["small_val"]
    mat = np.zeros((int(g["n_users"]), int(g["n_items"])), dtype=np.float32)
    mat[np.repeat(np.arange(mat.shape[0]), np.diff(ptr)), idx] = val
    att = _build(g, _DenseData(mat), gpu_device)
    att.margin_log = []
    ret = att.train_step(target_id_list=[0])
    run_min = att.run_margin_min()
    print(f"small case: device run-minimum margin {run_min:.3e}, reference {float(g['run_margin_min']):.3e}")
    assert float(g["run_margin_min"]) >= 20 * A_TOL
    assert run_min > 0.5 * float(g["run_margin_min"])
    dev_losses = _device_losses(att)
    print("phase losses device", dev_losses, "reference", g["phase_losses"])
    assert [n for n in g["phase_names"]] == ["pretrain_G", "train_D", "train_D", "train_G_adv", "train_G_attack", "train_G_attack"]
    assert np.allclose(dev_losses, g["phase_losses"], rtol=1e-4, atol=0)
    assert ret[0] == 0.0 == g["returned"][0] and abs(ret[1] - g["returned"][1]) <= 1e-4 * g["returned"][1]
    fake = att.generate_fake(target_id_list=[0])
    out = att.last_forward()
    print(f"final max |a_dev - a_ref| {np.abs(out['a'] - g['a']).max():.2e}")
    assert np.abs(out["a"] - g["a"]).max() <= 0.5 * float(g["run_margin_min"])
    assert np.array_equal(out["cls"], g["cls"]) and np.array_equal(out["value"], g["value"])
    fr, fc = np.nonzero(fake)
    assert np.array_equal(fr, g["fake_rows"]) and np.array_equal(fc, g["fake_cols"]) and np.array_equal(fake[fr, fc], g["fake_vals"])


def test_game_short_step_within_the_references_own_spread(gpu_device):
    """Measured on the MI355X: see the figures this test prints; DESIGN 8b records them."""
    g = np.load(os.path.join(GOLDEN, "aushplus_game_step.npz"))
    att = _build(g, _game(gpu_device), gpu_device)
    ret = att.train_step(target_id_list=[0])
    att._forward_templates()
    out = att.last_forward()
    dev_losses = _device_losses(att)
    gs, ds = att.generator_state(), att.discriminator_state()
    g_fp = np.asarray([_fp(gs[k].numpy()) for k in G_NAMES])
    d_fp = np.asarray([_fp(ds[k].numpy()) for k in D_NAMES])
    counts = np.bincount(out["cls"] + 1, minlength=6)
    differ = float((out["cls"] != g["cls"]).mean())
    print("phase losses device", dev_losses, "\nf32", g["phase_losses"], "\nf64", g["f64_phase_losses"])
    print("returned device", ret, "f32", g["returned"], "f64", g["f64_returned"])
    print("class counts device", counts, "f32", g["class_counts"], "f64", g["f64_class_counts"])
    print(f"entries in another class than the float32 reference: device {differ:.4f}, float64 reference "
          f"{float((g['f64_cls'] != g['cls']).mean()):.4f}")
    print("G fingerprints |device - f32|", np.abs(g_fp - g["g_fp"]).tolist(), "|f64 - f32|", np.abs(g["f64_g_fp"] - g["g_fp"]).tolist())
    print("D fingerprints |device - f32|", np.abs(d_fp - g["d_fp"]).tolist(), "|f64 - f32|", np.abs(g["f64_d_fp"] - g["d_fp"]).tolist())

    def within(dev, f32, f64, floor_rel, what):
        bound = np.maximum(3 * np.abs(np.asarray(f64) - np.asarray(f32)), floor_rel * np.abs(np.asarray(f32)))
        assert (np.abs(np.asarray(dev) - np.asarray(f32)) <= bound).all(), what

    within(dev_losses, g["phase_losses"], g["f64_phase_losses"], 1e-5, "phase losses")
    within(ret, g["returned"], g["f64_returned"], 1e-5, "returned tuple")
    within(g_fp, g["g_fp"], g["f64_g_fp"], 1e-4, "generator fingerprints")
    within(d_fp, g["d_fp"], g["f64_d_fp"], 1e-4, "discriminator fingerprints")
    within(counts, g["class_counts"], g["f64_class_counts"], 0.0, "template entries per class")
    assert differ <= 0.01
