"""CPU tests of AushPlus against the reference's own recorded run (tests/golden/aushplus_game_init.npz, written by
tests/golden/make_golden_aushplus.py): the template draw and the weight initialisation from the same seeds, and the float64
restatement the GPU tests lean on (tests/_aushplus_restate.py) against the reference's float32 values from the seeded init: a,
distribution and value at the template entries, the first pretrain_G batch's loss and parameter-gradient fingerprints, the
first train_D batch's loss.

Tolerances: the reference is float32, the restatement float64, so these are the single-step tolerances of
tests/test_aushplus_gpu.py (A_TOL 1e-5 for a, 1e-5 relative for a loss, 1e-4 relative for gradients, here on the recorded
fingerprints: the sum of squares within 2e-4 relative, the sum within 1e-4 of the gradient's L1 norm); class, distribution and
value exactly (the recorded margin at init is 0.35)."""
import os

import numpy as np
import torch

from recad_amd import dataset
from recad_amd.attack import aushplus as ap
from tests import _aushplus_restate as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G_NAMES = ("min_boundary_value", "interval_lengths", "layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias")
D_NAMES = ("main.0.weight", "main.0.bias", "main.2.weight", "main.2.bias", "main.4.weight", "main.4.bias")


def _fp(a):
    a = np.asarray(a, dtype=np.float64)
    return np.asarray([a.sum(), (a * a).sum()])


def _game_partial():
    g = np.load(os.path.join(GOLDEN, "aush_game_partial.npz"))
    full = dataset.from_config("explicit", "game", device="cpu", train_dict=g["train_kvr"], valid_dict=g["valid_kvr"],
                               test_dict=g["test_kvr"])
    np.random.seed(int(g["seed"]))
    return full.partial_sample(user_ratio=float(g["user_ratio"]))


def _setup():
    g = np.load(os.path.join(GOLDEN, "aushplus_game_init.npz"))
    ptr, idx, val = _game_partial().rating_csr()
    ptr, idx, val = np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(val, np.float32)
    assert [len(idx), idx.astype(np.float64).sum(), val.astype(np.float64).sum()] == g["csr_fp"].tolist()
    np.random.seed(int(g["seed"]))
    torch.manual_seed(int(g["seed"]))
    users, kept = ap.draw_templates(ptr, idx, val, 50, int(g["cfg_filler_num"]))
    gs, ds = ap.init_weights(int(g["n_items"]))
    return g, (ptr, idx, val), users, kept, gs, ds


def test_template_draw_and_weight_init_reproduce_the_reference():
    g, _, users, kept, gs, ds = _setup()
    assert np.array_equal(users, g["template_users"])
    assert np.array_equal(np.concatenate(kept), g["template_kept"])
    assert np.array_equal(np.cumsum([0] + [len(k) for k in kept]), g["template_kept_ptr"])
    lens = np.diff(g["template_kept_ptr"])
    assert lens.min() < 12 and lens.max() == 12                  # variable length is the normal case
    assert np.array_equal(np.concatenate([np.sort(k) for k in kept]), g["pos_cols"])
    for k, want in zip(G_NAMES, g["init_g_fp"]):
        assert np.allclose(_fp(gs[k].numpy()), want, rtol=1e-12, atol=0), k
    for k, want in zip(D_NAMES, g["init_d_fp"]):
        assert np.allclose(_fp(ds[k].numpy()), want, rtol=1e-12, atol=0), k


def test_restatement_against_the_reference_from_seeded_init():
    g, (ptr, idx, val), users, kept, gs, ds = _setup()
    trp = g["template_kept_ptr"]
    tcol = g["pos_cols"].astype(np.int64)
    tval = np.concatenate([val[ptr[u]:ptr[u + 1]][np.searchsorted(idx[ptr[u]:ptr[u + 1]], tcol[trp[r]:trp[r + 1]])]
                           for r, u in enumerate(users)])
    p = R.params64(gs)
    fw = R.g_forward(p, trp, tcol, tval)
    assert np.abs(fw["a"].detach().numpy() - g["a"]).max() <= 1e-5
    assert np.array_equal(fw["dist"].detach().numpy().astype(np.float32), g["dist"])
    assert np.array_equal(fw["masked"].detach().numpy().astype(np.float32), g["value"])
    assert float(fw["margin"].min()) >= 0.3 and float(g["margin_min"]) >= 0.3       # the fixture's is over all its forwards
    # the first pretrain_G batch
    rp, col, x = ap.gather_rows(ptr, idx, val, g["pretrain_users"])
    loss = R.ce_loss(R.g_forward(p, rp, col, x))
    loss.backward()
    assert abs(float(loss.detach()) - float(g["pretrain_loss"])) <= 1e-5 * float(g["pretrain_loss"])
    for k, want, amax in zip(G_NAMES, g["pretrain_grad_fp"], g["pretrain_grad_absmax"]):
        got = p[k].grad.numpy()
        assert abs((got * got).sum() - want[1]) <= 2e-4 * want[1], k
        assert abs(got.sum() - want[0]) <= 1e-4 * np.abs(got).sum(), k
        assert abs(np.abs(got).max() - amax) <= 1e-4 * amax, k
    # one Adam step of G (lr_g 0.01), then the first train_D batch: real rows = the batch's first attack_num users
    p2 = {k: torch.as_tensor(R.adam_first_step(v.detach().numpy(), v.grad.numpy(), 0.01)) for k, v in p.items()}
    fake = R.g_forward(p2, trp, tcol, tval)["masked"]
    d = R.params64(ds, grad=False)
    rp, col, x = ap.gather_rows(ptr, idx, val, g["d_users"][:50])
    d_loss = R.bce(R.d_forward(d, rp, col, x), 1.0) + R.bce(R.d_forward(d, trp, tcol, fake), 0.0)
    assert abs(float(d_loss) - float(g["d_loss"])) <= 1e-5 * float(g["d_loss"])
