"""CPU tests of tests/_pointwise_restate.py, the float64 restatement and the error budgets that test_ncf_kernels_gpu.py and
test_mf_kernels_gpu.py hold the NCF and MF kernels to: the restatement's whole-step gradients are torch's float64 autograd
gradients, a plain fp32 numpy implementation of every stage (its sums in index order and from the other end) stays inside every
budget on every case of the GPU tests, and six wrong implementations each break one by more than 2 x."""
import numpy as np
import pytest
import torch

from . import _pointwise_restate as R
from .test_gpu_parity import _torch_ncf

MODE_STR = {R.NEUMF: "NeuMF-end", R.MLP: "MLP", R.GMF: "GMF"}


def _relclose(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return np.max(np.abs(a - b)) <= tol * max(np.max(np.abs(b)), 1e-300) if a.size else True


def _drop_of(name, call=3):
    p = R.NCF_CASES[name][4]
    return (p, R.DROP_SEED, call) if p > 0 else None


# ================================================================ the restatement is the model
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mode", [R.NEUMF, R.MLP, R.GMF])
def test_ncf_restatement_is_autograd(mode, masked):
    f, L, p = 8, 3, 0.3
    c = R.ncf_case(f, L, mode, 37, seed=5 + mode)
    nb, w = c["nb"], R.widths(f, L)
    masks = [R.drop_mask(R.DROP_SEED, 0, l, (nb, w[l]), p) for l in range(L)] if masked else None
    leaves = [torch.tensor(np.asarray(t, dtype=np.float64), requires_grad=True) for t in R.ncf_tensors(c)]
    ug, ig, um, im = leaves[:4]
    W, b, pw, pb = leaves[4:4 + L], leaves[4 + L:4 + 2 * L], leaves[4 + 2 * L].view(1, -1), leaves[5 + 2 * L]
    u, i = torch.from_numpy(c["users"]), torch.from_numpy(c["items"])
    drop = (p, [torch.from_numpy(m.astype(np.float64)) for m in masks]) if masked else None
    logit = _torch_ncf((ug, ig, um, im, W, b, pw, pb), MODE_STR[mode], f, L, u, i, drop=drop)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, torch.from_numpy(c["labels"].astype(np.float64)))
    loss.backward()
    got_loss, grads = R.ncf_step64(c, masks, p if masked else 0.0)
    assert abs(got_loss - loss.item()) <= 1e-12 * loss.item()
    for k, (g, leaf) in enumerate(zip(grads, leaves)):
        want = np.zeros(leaf.numel()) if leaf.grad is None else leaf.grad.numpy().reshape(-1)
        assert _relclose(g, want), (k, R.MODE_NAMES[mode])
    if not masked:
        assert abs(logit[0].item() - R.BIG) < 0.6 and abs(logit[1].item() + R.BIG) < 0.6, "the +-40 pairs are not there"


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_mf_restatement_is_autograd(p):
    c = R.mf_case(13, 41, seed=3)
    nb = c["nb"]
    drop = (p, R.DROP_SEED, 2) if p > 0 else None
    ref = R.mf_step(c, drop)
    leaves = [torch.tensor(np.asarray(c[k], dtype=np.float64), requires_grad=True) for k in ("ue", "ie", "ub", "ib")]
    u, i = torch.from_numpy(c["users"]), torch.from_numpy(c["items"])
    x = (leaves[0][u] * leaves[1][i]).sum(1) + leaves[2][u] + leaves[3][i] + float(np.float32(c["mean"]))
    if drop is not None:
        assert 0 < ref["keep"].sum() < nb
        x = x * torch.from_numpy(ref["keep"].astype(np.float64)) * float(R.drop_scale(p))
    loss = torch.nn.functional.binary_cross_entropy_with_logits(x, torch.from_numpy(c["labels"].astype(np.float64)))
    loss.backward()
    assert abs(ref["loss"] - loss.item()) <= 1e-12 * loss.item()
    for (g, _), leaf in zip(ref["grad"], leaves):
        assert _relclose(g, leaf.grad.numpy())
    if drop is None:
        assert abs(ref["x"][0] - R.BIG) < 1e-3 and abs(ref["x"][1] + R.BIG) < 1e-3


# ================================================================ correct fp32 fits every budget
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", list(R.NCF_CASES))
def test_ncf_fp32_inside_every_bound(name, reverse):
    c, drop = R.named_case(name), _drop_of(name)
    r = R.check_ncf_step(c, R.ncf_step32(c, drop, reverse=reverse), drop)
    r.update({"scoring." + k: v for k, v in R.check_ncf_forward(c, R.ncf_step32(c, None, reverse=reverse), None).items()})
    assert max(r.values()) <= 1.0, {k: v for k, v in r.items() if v > 1.0}
    f, L, mode, nb, p = R.NCF_CASES[name]
    stages = {"predict.d0", "predict.loss", "wgrad.pw", "wgrad.pb"}
    if mode != R.GMF:
        stages |= {"gather", "predict.dxl", "scatter.um", "scatter.im", "scatter.untouched"} | {f"forward.{l}" for l in range(L)}
        stages |= {f"backward.{l}.{k}" for l in range(L) for k in ("dX", "dW", "db")}
    stages |= {"unused.gmf"} if mode == R.MLP else {"predict.g_ug", "predict.g_ig", "predict.gmf_untouched"}
    stages |= {"unused.tower"} if mode == R.GMF else set()
    assert stages <= set(r), stages - set(r)


def test_ncf_cases_hold_what_they_promise():
    c = R.named_case("C")
    u, i = c["users"], c["items"]
    assert np.bincount(u).max() == R.HUB_USER and np.bincount(i).max() == R.HUB_ITEM
    assert len(np.unique(u)) == c["nb"] - R.HUB_USER + 1 and len(np.unique(i)) == c["nb"] - R.HUB_ITEM + 1
    assert c["n_users"] > len(np.unique(u)) and c["n_items"] > len(np.unique(i)), "no untouched row"
    for name in ("B", "C", "Dgmf", "Dmlp", "E", "A5"):
        c = R.named_case(name)
        s, _ = R.logits(c["P"], c["mode"], c["f"], c["users"], c["items"], R.ncf_step32(c)["acts"][c["L"]] if c["mode"] != R.GMF else None)
        assert abs(s[0] - R.BIG) < 0.6 and abs(s[1] + R.BIG) < 0.6, (name, s[:2])
    d = R.named_case("A3")
    assert len(np.unique(d["users"])) == 3 and not d["big"]
    # the dropout restated here is the one test_gpu_parity.py restates
    from ._drop_restate import _drop_keep, _step_seed
    assert np.array_equal(R.drop_mask(7, 2, 1, (5, 8), 0.3), _drop_keep(_step_seed(7, 2 * 16 + 1), 40, 1.0 - float(np.float32(0.3))).reshape(5, 8))
    assert R.score_call(3, 2) * 16 >= 1 << 64, "the scoring call number wraps in 64 bits: drop_mask must wrap too"


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("p", R.MF_DROPS)
@pytest.mark.parametrize("nb", R.MF_NB)
@pytest.mark.parametrize("dim", R.MF_DIMS)
def test_mf_fp32_inside_every_bound(dim, nb, p, reverse):
    c = R.named_mf_case(dim, nb)
    drop = (p, R.DROP_SEED, 5) if p > 0 else None
    g, loss = R.mf_step32(c, drop, reverse=reverse)
    r = R.check_mf_step(c, g, loss, drop)
    assert max(r.values()) <= 1.0, {k: v for k, v in r.items() if v > 1.0}
    if drop is not None and nb >= 5:
        keep = R.mf_step(c, drop)["keep"]
        assert 0 < keep.sum() < nb


def test_mf_dropped_sample_is_log2_and_zero():
    c = R.mf_case(7, 1, seed=1, hubs=False)
    step = next(s for s in range(64) if not R.mf_step(c, (0.25, R.DROP_SEED, s))["keep"][0])
    ref = R.mf_step(c, (0.25, R.DROP_SEED, step))
    assert abs(ref["loss"] - np.log(2.0)) < 1e-15 and all(not g.any() and not b.any() for g, b in ref["grad"])
    g, loss = R.mf_step32(c, (0.25, R.DROP_SEED, step))
    assert not np.any(R.bits(g)) and max(R.check_mf_step(c, g, loss, (0.25, R.DROP_SEED, step)).values()) <= 1.0


# ================================================================ wrong implementations break a budget by more than 2 x
def _worst(r):
    k = max(r, key=r.get)
    return k, r[k]


@pytest.mark.parametrize("mutate,name,stage", [
    ("scatter_pair", "C", "scatter.um"),            # one pair dropped from a scatter
    ("scatter_pair", "A5", "scatter.um"),
    ("last_slab", "C", "wgrad.pw"),                 # the last slab (8 rows of 200) dropped from the predict weight gradient
    ("last_slab", "A65", "wgrad.pb"),               # ... a slab of one row
    ("pre_dropout_mask", "Cdrop", "backward.1.dX"),  # a ReLU gate taken from the activation before its dropout
    ("pw_halves", "C", "predict.d0"),               # the GMF and the MLP half of pw swapped
    ("seed_layer", "Cdrop", "gather"),              # layer 1's dropout seed on layer 0
])
def test_ncf_mutations_break_a_bound(mutate, name, stage):
    c, drop = R.named_case(name), _drop_of(name)
    good = R.check_ncf_step(c, R.ncf_step32(c, drop), drop)
    assert max(good.values()) <= 1.0
    bad = R.check_ncf_step(c, R.ncf_step32(c, drop, mutate=mutate), drop)
    assert bad[stage] > 2.0, (stage, bad[stage], _worst(bad))
    # and only the stages fed by the wrong one notice: every stage is checked on its own inputs
    if mutate in ("scatter_pair", "last_slab"):
        assert all(v <= 1.0 for k, v in bad.items() if not k.startswith(stage.split(".")[0])), bad


def test_short_last_step_divides_by_its_own_length():
    """1 / batch in place of 1 / nb on the 16-pair tail of a 32-pair epoch"""
    c = R.sub_case(R.named_case("A64"), 32, 48)
    assert max(R.check_ncf_step(c, R.ncf_step32(c)).values()) <= 1.0
    bad = R.check_ncf_step(c, R.ncf_step32(c, nb_div=32))
    assert bad["predict.d0"] > 2.0 and bad["predict.loss"] > 2.0
    m = R.sub_case(R.named_mf_case(63, 1100), 1088, 1100)
    g, loss = R.mf_step32(m, nb_div=64)
    bad = R.check_mf_step(m, g, loss)
    assert bad["mf.g_ue"] > 2.0 and bad["mf.loss"] > 2.0
    g, loss = R.mf_step32(m, mutate="scatter_pair")
    assert R.check_mf_step(m, g, loss)["mf.g_ue"] > 2.0
