"""GPU tests of the PGA attacker end to end (recad_amd/attack/pga.py) on the 300 x 120 synthetic set of tests/test_apr_gpu.py with
seeded 1..5 ratings: three train_steps against the restatement chained from the device's own tables, generate_fake, run-to-run
bit-identity, and the "no defense", "sweep" and "defense" workflows.

Tolerances of the chained check.  The class does not keep D, so g is held to the float64 D of the float64 scores of the device's
tables: a score computed by the fp32 GEMM is within delta_u = gamma_{d + 1} max_j |x_u| . |y+_j| of it, the softmax moves by at
most 2.1 delta_u p_uj, so g gets gamma-budget + sum_u 2.1 delta_u p_uj |x_uk| / |E_t|; the loss is 1-Lipschitz in the scores' sup
norm twice over (lse and s_t): 2 max_u delta_u per target.  Z, M, h, V and grad are held stage by stage from the device's own
upstream outputs as in tests/test_pga_kernels_gpu.py (Z and V to the hard bound here: the walk needs the systems the device
built, which the class does not keep).  The update and the selection are exact."""
import numpy as np
import pytest
import torch

from recad_amd import dataset, model, synth, workflow
from tests import _ials_restate as IR
from tests import _pga_restate as P
from tests import test_apr_gpu as A
from tests import test_ials_gpu as IA

pytestmark = pytest.mark.gpu
U, I = A.U, A.I
CFG = dict(attack_num=10, filler_num=8, factor_num_s=16, alpha_s=40.0, reg_lambda_s=10.0, init_sweeps_s=3, sweeps_s=2, seed_s=5, lr=0.25)


def _explicit(dev):
    r = synth.with_ratings(dict(A._data(), n_users=U, n_items=I), seed=7)
    return dataset.from_config("explicit", "small", train_csr=r["train"], valid_csr=r["valid"], test_csr=r["test"], device=dev), r["train"]


def _pga(dev, ds, np_seed=3, **kw):
    np.random.seed(np_seed)
    return model.from_config("attacker", "pga", device=dev, **{**CFG, **kw}).I(dataset=ds)


@pytest.mark.parametrize("targets", [[A.TARGET], [A.TARGET, 3, 40]], ids=["one-target", "three-targets"])
def test_three_train_steps_against_the_chained_restatement(gpu_device, targets):
    ds, (ptr, idx, val) = _explicit(gpu_device)
    ptr, idx, val = np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(val, np.float32)
    att = _pga(gpu_device, ds)
    att.user_block = 128                                    # three blocks of users, the last one short
    d, Af, F, w, alpha, lam = 16, CFG["attack_num"], CFG["filler_num"], att.wbar, 40.0, 10.0
    R = att.strengths()
    assert set(np.unique(R)) <= {0.0, 1.0} and np.all(R.sum(axis=1) == F), "the templates"
    R[:, targets] = 1.0
    losses = []
    for step in range(3):
        cols = P.select(R, targets, F)
        (loss,) = att.train_step(target_id_list=targets)
        losses.append(loss)
        t, st, grad = att.surrogate_tables(), att.last_stages(), att.last_gradient()
        X, Yo, Yp = t["X"], t["Yo"], t["Yp"]
        # the fake rows of X and the items of Yp solve the systems of the profile the step started from (hard bound)
        cp, ci, cv = P.combined_csr(ptr, idx, val, cols, 5.0)
        Go = IR.gram64(Yo, lam)
        for f in range(Af):
            A64, b64 = IR.system64(Go, Yo, cols[f], np.full(len(cols[f]), 5.0, np.float32), alpha)
            x = IR.solve64(A64, b64)
            assert np.abs(X[U + f] - x).max() <= IR.x_hard(A64, x, Yo, cols[f], np.full(len(cols[f]), 5.0, np.float32), alpha, I)[1], (step, f)
        tp = IR.transpose(cp, ci, cv, I)
        Gx = IR.gram64(X, lam)
        for j in list(targets) + [0, I - 1]:
            sl = slice(tp[0][j], tp[0][j + 1])
            A64, b64 = IR.system64(Gx, X, tp[1][sl], tp[2][sl], alpha)
            y = IR.solve64(A64, b64)
            assert np.abs(Yp[j] - y).max() <= IR.x_hard(A64, y, X, tp[1][sl], tp[2][sl], alpha, U + Af)[1], (step, j)
        # the loss and g from the float64 scores of the device's tables
        S = X[:U].astype(np.float64) @ Yp.astype(np.float64).T
        delta = P.gamma(d + 1) * (np.abs(X[:U].astype(np.float64)) @ np.abs(Yp.astype(np.float64)).T).max(axis=1)
        want, g64, e_g, Ds = 0.0, 0.0, 0.0, []
        for tt in targets:
            e = P.eligible(ptr, idx, U, tt)
            inv = 1.0 / e.sum()
            D64, terms = P.loss_stage64(S, ptr, idx, 0, tt, e, inv)
            want += terms.sum()
            prob = D64 / inv
            prob[e, tt] += 1.0
            e_g = e_g + (2.1 * delta[:, None] * prob * inv + P.U24 * np.abs(D64)).T @ np.abs(X[:U].astype(np.float64))
            Ds.append(D64)
        g64 = P.g_stage64(Ds, [X[:U]] * len(Ds))
        e_g = e_g + P.g_budget(Ds, [X[:U]] * len(Ds))
        assert abs(loss - want) <= len(targets) * 2.0 * delta.max() + 2.0 ** -40 * abs(want), (step, loss, want)
        assert np.all(np.abs(st["g"] - g64) <= e_g), step
        # the hypergradient, stage by stage from the device's own outputs
        Z64 = P.solve_stage64(X, lam, *tp, alpha, st["g"])
        for j in range(I):
            sl = slice(tp[0][j], tp[0][j + 1])
            A64, _ = IR.system64(Gx, X, tp[1][sl], tp[2][sl], alpha)
            assert np.abs(st["Z"][j] - Z64[j]).max() <= P.hard_rhs(A64, Z64[j], sl.stop - sl.start, U + Af)[1], (step, j)
        assert np.all(np.abs(st["M"] - P.m_stage64(st["Z"], Yp)) <= P.m_budget(st["Z"], Yp))
        assert np.all(np.abs(st["H"] - P.h_stage64(st["Z"], Yp, X[U:], st["M"], cols, w)) <= P.h_budget(st["Z"], Yp, X[U:], st["M"], cols, w))
        fp, fi, fv = P.fake_csr(cols, 5.0)
        V64 = P.solve_stage64(Yo, lam, fp, fi, fv, alpha, st["H"])
        for f in range(Af):
            A64, _ = IR.system64(Go, Yo, cols[f], fv[:len(cols[f])], alpha)
            assert np.abs(st["V"][f] - V64[f]).max() <= P.hard_rhs(A64, V64[f], len(cols[f]), I)[1], (step, f)
        assert np.all(np.abs(grad - P.grad_stage64(X[U:], st["V"], st["Z"], Yp, Yo, w)) <= P.grad_budget(X[U:], st["V"], st["Z"], Yp, Yo, w))
        # the update, the pinning and the new profiles: exact
        R = P.update_walk(R, grad, P.max_abs_bits(grad), CFG["lr"], targets)
        assert np.array_equal(att.strengths().view(np.uint32), R.view(np.uint32)), step
        assert np.array_equal(att.profiles(), P.select(R, targets, F)), step
    assert att.last_loss == losses[-1] and all(np.isfinite(losses))
    print(f"adversarial loss over three steps ({len(targets)} targets): {losses}")


def test_generate_fake_rows(gpu_device):
    ds, _ = _explicit(gpu_device)
    targets = [A.TARGET, 3, 40]
    att = _pga(gpu_device, ds)
    before = att.generate_fake(target_id_list=targets)               # before any train_step: the templates' profiles
    att.train_step(target_id_list=targets)
    for fake in (before, att.generate_fake(target_id_list=targets)):
        assert fake.shape == (10, I) and fake.dtype == np.float32 and set(np.unique(fake)) <= {0.0, 5.0}
        rate = 10 // 3
        for r in range(10):
            share = [t for i, t in enumerate(targets) if i * rate <= r < (i + 1) * rate]
            assert np.count_nonzero(fake[r]) == CFG["filler_num"] + len(share), r
            assert all(fake[r, t] == 5 for t in share) and all(fake[r, t] == 0 for t in targets if t not in share)
    prof = att.profiles()
    fillers = [sorted(set(prof[r]) - set(targets)) for r in range(10)]
    assert all(sorted(np.nonzero(fake[r])[0].tolist()) == sorted(fillers[r] + [t for t in targets if fake[r, t]]) for r in range(10))
    odd = model.from_config("attacker", "pga", device=gpu_device, **{**CFG, "fake_rating": 4}).I(dataset=ds)
    out = odd.generate_fake(target_id_list=[A.TARGET])
    assert set(np.unique(out)) == {0.0, 4.0, 5.0} and np.all(out[:, A.TARGET] == 5)


def test_two_runs_from_one_seed_give_the_same_bits(gpu_device):
    ds, _ = _explicit(gpu_device)
    runs = []
    for _ in range(2):
        att = _pga(gpu_device, ds)
        losses = [att.train_step(target_id_list=[A.TARGET])[0] for _ in range(2)]
        runs.append((losses, att.strengths(), att.profiles(), att.last_gradient(), att.surrogate_tables()["Yp"], att.generate_fake(target_id_list=[A.TARGET])))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    assert not np.array_equal(_pga(gpu_device, ds, np_seed=4).strengths(), _pga(gpu_device, ds).strengths()), "another seed, other templates"


def test_refusals_at_train_step_launch_nothing(gpu_device):
    ds, (ptr, idx, _) = _explicit(gpu_device)
    att = _pga(gpu_device, ds)
    R = att.strengths()
    for bad, msg in (([], "empty"), ([I], "must lie in"), ([1, 1], "repeats")):
        with pytest.raises(ValueError, match=msg):
            att.train_step(target_id_list=bad)
    assert np.array_equal(att.strengths(), R) and att.last_loss is None and att._tables is None


# ------------------------------------------------------------------------------------------------------------ the workflows
def test_no_defense_workflow_against_ials(gpu_device):
    explicit, _ = _explicit(gpu_device)
    wf = workflow.from_config("no defense", victim_data=IA._small(gpu_device), attack_data=explicit, victim=IA._lazy(),
                              attacker=model.from_config("attacker", "pga", device=gpu_device, **CFG), rec_epoch=2, attack_epoch=2,
                              device=gpu_device, target_id_list=[A.TARGET], topks=[5, 10, 20])
    res = wf.execute()
    assert wf.fake_dataset.n_users == U + CFG["attack_num"] and res["n_eval_users"] > 0
    assert all(np.isfinite(v) for v in res.values()), res
    assert wf.attacker.last_loss is not None and np.isfinite(wf.attacker.last_loss)


def test_two_cases_of_a_sweep_against_apr(gpu_device):
    explicit, _ = _explicit(gpu_device)
    cases = [{"attacker": model.from_config("attacker", "pga", device=gpu_device, **CFG), "target_id_list": [A.TARGET]},
             {"attacker": model.from_config("attacker", "pga", device=gpu_device, **{**CFG, "attack_num": 12}), "target_id_list": [3, 40]}]
    torch.manual_seed(5)
    wf = workflow.from_config("sweep", victim_data=A._small(gpu_device), attack_data=explicit, victim=A._lazy(adv_start_epoch=1), cases=cases,
                              rec_epoch=2, attack_epoch=2, device=gpu_device, topks=[5, 10, 20], group=2)
    res = wf.execute()
    assert len(res) == 2 and [d.n_users for d in wf.fake_datasets] == [U + 10, U + 12]
    assert all(np.isfinite(v) for r in res for v in r.values()), res


def test_defense_workflow_with_knn_defender(gpu_device):
    explicit, _ = _explicit(gpu_device)
    defender = model.from_config("defender", "KnnSelectUsers", k=25, attack_num=CFG["attack_num"], device=gpu_device)
    wf = workflow.from_config("defense", victim_data=IA._small(gpu_device), attack_data=explicit, victim=IA._lazy(),
                              attacker=model.from_config("attacker", "pga", device=gpu_device, **CFG), defender=defender, rec_epoch=2,
                              attack_epoch=1, device=gpu_device, target_id_list=[A.TARGET], topks=[10, 20])
    res = wf.execute()
    assert set(res) == {"attacked", "defended", "n_flagged"} and wf.fake_dataset.n_users == U + CFG["attack_num"]
    assert all(np.isfinite(v) for part in ("attacked", "defended") for v in res[part].values()), res
