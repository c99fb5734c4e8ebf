"""CPU tests of the PCASelectUsers defender (recad_amd/defense): the reference's counting rules, the sign
convention, the registry / lazy-init contract, the workflow hook, the golden fixture's own consistency, and the block-width
rule against a numpy restatement of the solver (tests/_pca_restate.py)."""
import os

import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, model, synth, workflow
from recad_amd.defense.pca_select_users import block_width, effective_k, flag_count, sign_fix
from recad_amd.utils import NotInstantiatedError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _reference_count(attack_num, U):
    """PCASelectUsers.py:34,85-90 as written: while i < attack_ratio * len(disSort)."""
    ratio, i = attack_num / U, 0
    while i < ratio * U:
        i += 1
    return i


def test_flag_count_rule():
    over = [U for U in range(51, 4000) if (50 / U) * U > 50]
    assert over, "some U must round (50 / U) * U above 50"
    for U in over[:5] + [51, 100, 3229, 5950]:
        assert flag_count(50, U) == _reference_count(50, U)
    assert flag_count(50, over[0]) == 51
    assert flag_count(50, 3229) == 50 and flag_count(0, 10) == 0 and flag_count(20, 10) == 10


def test_k_reset_rule():
    assert effective_k(3, 100, 50) == 3
    assert effective_k(50, 100, 50) == 3 and effective_k(49, 100, 50) == 49
    assert effective_k(10 ** 6, 512, 511) == 3


def test_sign_convention():
    v = np.array([[0.1, -0.5, 0.3], [-0.7, 0.5, -0.3], [0.2, 0.1, 0.0]], dtype=np.float32)
    out = sign_fix(v)
    # column 0: largest |x| is -0.7 -> flipped; column 1: tie between -0.5 (row 0) and 0.5 -> lowest index wins -> flipped;
    # column 2: tie 0.3 (row 0) / -0.3 -> kept
    assert np.array_equal(out, v * np.array([-1, -1, 1], dtype=np.float32))
    t = sign_fix(torch.from_numpy(v))
    assert torch.equal(t, torch.from_numpy(out))
    assert np.array_equal(sign_fix(out), out)


def test_registry_and_lazy_init():
    assert model.factories["defender"]["PCASelectUsers"] is not None
    cfg = default.MODEL["defender"]["PCASelectUsers"]
    assert cfg["kVals"] == 3 and cfg["attack_num"] == 50
    assert {"block", "tol", "max_iter", "seed"} <= set(cfg)
    lazy = model.from_config("defender", "PCASelectUsers", attack_num=15, not_a_key=1)
    assert lazy.model_name == "PCASelectUsers"
    assert lazy._init_config["attack_num"] == 15 and lazy._init_config["kVals"] == 3 and "not_a_key" not in lazy._init_config
    for call in (lambda: lazy.defense_step(), lambda: lazy.input_describe()):
        with pytest.raises(NotInstantiatedError):
            call()
    d = synth.make("tiny")
    ds = dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                             need_graph=False, device=torch.device("cpu"), seed=5)
    real = lazy.I(dataset=ds)
    assert real.I() is real and real.user_num == ds.n_users and real.item_num == ds.n_items
    assert "dataset" in real.input_describe()["defense_step"]
    assert real.reset(attack_num=7)._init_config["attack_num"] == 7
    with pytest.raises(_lib.HipCallError):
        real.defense_step()      # CPU device: no fallback


def test_workflow_passes_the_poisoned_dataset_cpu():
    from tests.test_host_logic import _StubVictim

    class Seer:
        def __init__(self):
            self.seen = None

        def I(self, **kw):
            return self

        def to(self, device):
            return self

        def input_describe(self):
            return {"defense_step": {"dataset": None}}

        def defense_step(self, dataset=None):
            self.seen = dataset
            return list(range(dataset.n_users - 10, dataset.n_users))

    d = synth.make("tiny")
    ds = dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                             need_graph=False, device=torch.device("cpu"), seed=5)
    seer = Seer()
    wf = workflow.from_config("defense", victim_data=ds, attack_data=None, victim=_StubVictim(),
                              attacker=workflow.RandomAttack(ds.n_items, attack_num=10, filler_num=5, seed=1),
                              defender=seer, rec_epoch=1, attack_epoch=0, device=torch.device("cpu"))
    res = wf.execute()
    assert seer.seen is wf.fake_dataset and seer.seen.n_users == ds.n_users + 10
    assert res["n_flagged"] == 10


def _dense_cov(g):
    U, I = int(g["n_users"]), int(g["n_items"])
    A = np.zeros((U, I), dtype=np.float64)
    rows = np.repeat(np.arange(U), np.diff(g["ptr"]))
    A[rows, g["idx"]] = g["val"]
    var = A.var(axis=0)
    var = np.where(var.astype(np.float32) < 10 * np.finfo(np.float32).eps, 1.0, var)
    S = A / np.sqrt(var)
    return A, S.T @ S


@pytest.mark.parametrize("name", ["pca_game_fake50", "pca_dev_kreset"])
def test_golden_fixture_is_consistent(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    U, I = int(g["n_users"]), int(g["n_items"])
    assert len(g["ptr"]) == U + 1 and g["ptr"][-1] == len(g["idx"]) == len(g["val"])
    assert int(g["k"]) == effective_k(int(g["kVals"]), U, I) == 3
    A, C = _dense_cov(g)
    lam = np.linalg.eigh(C)[0][::-1][: int(g["k"])]
    assert np.allclose(g["vals"], lam, rtol=1e-4), (g["vals"], lam)
    assert np.allclose(g["vals_conv"], lam, rtol=1e-4)
    assert np.array_equal(sign_fix(g["vecs_conv"]), g["vecs_conv"])
    a, b = g["vecs"].astype(np.float64), g["vecs_conv"].astype(np.float64)
    cos = np.abs((a * b).sum(0)) / (np.linalg.norm(a, axis=0) * np.linalg.norm(b, axis=0))
    assert np.all(cos >= 1 - 1e-5), cos
    # the reference's distances under the convention: (A o A) . sum_j v_j
    dist = (A ** 2) @ g["vecs_conv"].astype(np.float64).sum(axis=1)
    assert np.allclose(dist, g["dist_conv"], atol=1e-4 * np.abs(dist).max())
    m = flag_count(int(g["attack_num"]), U)
    assert len(g["spam"]) == len(g["spam_conv"]) == m
    assert g["spam_conv"].tolist() == np.argsort(g["dist_conv"], kind="stable")[:m].tolist()


def test_block_width_rule():
    assert [block_width(k) for k in (1, 2, 3)] == [8, 8, 8], "kVals <= 3 keeps the 8-wide block its fixtures were recorded with"
    assert all(block_width(k) == 16 for k in range(4, 17))
    for k in (0, 17, 100):
        with pytest.raises(ValueError, match="kVals"):
            block_width(k)
    assert default.MODEL["defender"]["PCASelectUsers"]["block"] is None, "the default configuration uses the rule"


_RESTATED = [("pca_dev_kreset", k) for k in range(1, 17)] + [("pca_game_fake50", k) for k in (3, 8, 15, 16)]


@pytest.mark.parametrize("name,k", _RESTATED)
def test_block_width_converges_in_the_restatement(name, k):
    """The width block_width(k) picks reaches the default tol within the default max_iter on both stored matrices, in the numpy
    restatement of subspace_eigs (fp64 arithmetic, V / T / W rounded to fp32).  dev at every kVals (it is small, and the slowest:
    203 and 211 iterations at 15 and 16, 165 at 3), game at the two slowest (121 and 230 at 15 and 16) and two easy ones."""
    from tests._pca_restate import golden_operator, subspace_eigs_restated

    cfg = default.MODEL["defender"]["PCASelectUsers"]
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    apply, U, I = golden_operator(g)
    assert effective_k(k, U, I) == k
    lam, it, res = subspace_eigs_restated(apply, I, k, block_width(k), tol=cfg["tol"], max_iter=cfg["max_iter"], seed=cfg["seed"])
    assert it is not None, f"{name} kVals {k} block {block_width(k)}: residuals / lambda_1 {res} after {cfg['max_iter']} iterations"
    assert np.allclose(lam[: min(k, 3)], g["vals_conv"][: min(k, 3)], rtol=1e-4), "the restatement solves the fixture's problem"


def test_eight_wide_block_stalls_at_k5_in_the_restatement():
    """Why the rule switches to 16 at kVals = 4 and not at 6: with three guard vectors dev's fifth eigenpair (lambda_5 / lambda_6
    = 1.0014, lambda_9 / lambda_5 = 0.977) is still at 4e-4 * lambda_1 after 300 iterations, and kVals = 4 needs 241 of them."""
    from tests._pca_restate import golden_operator, subspace_eigs_restated

    apply, U, I = golden_operator(np.load(os.path.join(GOLDEN, "pca_dev_kreset.npz")))
    _, it, res = subspace_eigs_restated(apply, I, 5, 8)
    assert it is None and res.max() > 1e-4, (it, res)
    _, it4, _ = subspace_eigs_restated(apply, I, 4, 8)
    _, it16, _ = subspace_eigs_restated(apply, I, 5, 16)
    assert it4 is not None and it4 > 200 and it16 is not None and it16 < 60, (it4, it16)
