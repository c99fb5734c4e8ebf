"""GPU tests of the PCASelectUsers defender (csrc/pca.hip + recad_amd/defense): against the reference's own run on
the game data (tests/golden/make_golden_pca.py), fp64 residuals at the ml1m / yelp / config-4 shapes, determinism,
failure modes and the defence workflow."""
import os
import time

import numpy as np
import pytest
import torch

from recad_amd import dataset, model, synth, workflow
from recad_amd.defense.pca_select_users import flag_count

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _defender(data, dev, **kw):
    return model.from_config("defender", "PCASelectUsers", device=dev, **kw).I(dataset=data)


def _cos(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a * b).sum(0) / (np.linalg.norm(a, axis=0) * np.linalg.norm(b, axis=0))


@pytest.mark.parametrize("name", ["pca_game_fake50", "pca_dev_kreset"])
def test_against_reference(gpu_device, name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    U, I, m = int(g["n_users"]), int(g["n_items"]), flag_count(int(g["attack_num"]), int(g["n_users"]))
    # dev's third eigengap is 1.7 % of lambda_1, so an eigenvector's error is ~60x its residual: the default tol = 1e-5 leaves
    # distances 1.04x the 1e-4 tolerance away from ARPACK's; tol = 1e-6 (a build key) puts them 7x inside it
    extra = {"tol": 1e-6} if name == "pca_dev_kreset" else {}
    d = _defender((g["ptr"], g["idx"], g["val"], I), gpu_device, kVals=int(g["kVals"]), attack_num=int(g["attack_num"]), **extra)
    spam = d.defense_step()
    assert d.k == int(g["k"]) == 3
    assert np.allclose(d.eigenvalues, g["vals"], rtol=1e-4), (d.eigenvalues, g["vals"])
    vecs = d.eigenvectors.cpu().numpy()
    assert np.all(np.abs(_cos(vecs, g["vecs"])) >= 1 - 1e-5), _cos(vecs, g["vecs"])
    assert np.all(_cos(vecs, g["vecs_conv"]) >= 1 - 1e-5), _cos(vecs, g["vecs_conv"])
    dist = d.distances.cpu().numpy().astype(np.float64)
    tol = 1e-4 * np.abs(g["dist_conv"]).max()
    assert np.abs(dist - g["dist_conv"]).max() <= tol
    assert len(spam) == m == len(g["spam_conv"])
    dm = np.sort(g["dist_conv"], kind="stable")[m - 1]
    for u in set(spam) ^ set(g["spam_conv"].tolist()):
        assert abs(g["dist_conv"][u] - dm) <= tol, (u, g["dist_conv"][u], dm)
    assert d.predLabels.sum() == m and [u for u, _ in d.disSort[:m]] == spam
    assert all(d.disSort[i][1] <= d.disSort[i + 1][1] for i in range(U - 1))


def _fp64_residuals(U, I, rowptr, col, val, lam, vecs):
    """||C v_j - lambda_j v_j|| with C = D^-1 A^T A D^-1 in fp64 (torch.sparse), D from the test's own column variances."""
    dev = vecs.device
    rows = torch.repeat_interleave(torch.arange(U, device=dev), (rowptr[1:] - rowptr[:-1]).long())
    v64 = val.double()
    s1 = torch.zeros(I, dtype=torch.float64, device=dev).index_add_(0, col.long(), v64)
    s2 = torch.zeros(I, dtype=torch.float64, device=dev).index_add_(0, col.long(), v64 * v64)
    var = s2 / U - (s1 / U) ** 2
    var = torch.where(var.float() < 10 * torch.finfo(torch.float32).eps, torch.ones_like(var), var)
    inv = 1.0 / torch.sqrt(var)
    A = torch.sparse_coo_tensor(torch.stack([rows, col.long()]), v64, (U, I)).coalesce()
    At = A.t().coalesce()
    V = vecs.double()
    CV = inv[:, None] * torch.sparse.mm(At, torch.sparse.mm(A, inv[:, None] * V))
    lam_t = torch.as_tensor(lam, dtype=torch.float64, device=dev)
    return torch.linalg.norm(CV - V * lam_t[None, :], dim=0).cpu().numpy(), CV


def _synth_csr(name, dev):
    d = synth.make_device(name, dev)
    ptr, idx = d["train"]
    return d["n_users"], d["n_items"], ptr.to(torch.int32), idx, torch.ones(idx.numel(), dtype=torch.float32, device=dev)


@pytest.mark.parametrize("name", ["ml1m", "yelp"])
def test_fp64_residuals_at_scale(gpu_device, name):
    U, I, rp, col, val = _synth_csr(name, gpu_device)
    d = _defender((rp, col, val, I), gpu_device, attack_num=50)
    spam = d.defense_step()
    assert len(spam) == flag_count(50, U)
    res, _ = _fp64_residuals(U, I, rp, col, val, d.eigenvalues, d.eigenvectors)
    assert np.all(res <= d.tol * d.eigenvalues[0]), (res / d.eigenvalues[0], d.iterations)
    if name == "ml1m":
        rows = torch.repeat_interleave(torch.arange(U, device=gpu_device), (rp[1:] - rp[:-1]).long())
        A = torch.zeros(U, I, dtype=torch.float64, device=gpu_device)
        A[rows, col.long()] = 1.0
        var = A.var(dim=0, unbiased=False)
        var = torch.where(var.float() < 10 * torch.finfo(torch.float32).eps, torch.ones_like(var), var)
        S = A / torch.sqrt(var)
        lam = torch.linalg.eigvalsh(S.t() @ S).flip(0)[:3].cpu().numpy()
        assert np.allclose(d.eigenvalues, lam, rtol=1e-5), (d.eigenvalues, lam)


def test_config4_shape_sparse_only(gpu_device):
    U, I, rp, col, val = _synth_csr("config4", gpu_device)
    d = _defender((rp, col, val, I), gpu_device, attack_num=50)
    t0 = time.perf_counter()
    spam = d.defense_step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    assert elapsed < 120.0, f"config-4 defense_step took {elapsed:.1f} s ({d.iterations} iterations)"
    assert len(spam) == flag_count(50, U)
    res, _ = _fp64_residuals(U, I, rp, col, val, d.eigenvalues, d.eigenvectors)
    assert np.all(res <= d.tol * d.eigenvalues[0]), (res / d.eigenvalues[0], d.iterations)


def test_determinism_and_failure_modes(gpu_device):
    g = np.load(os.path.join(GOLDEN, "pca_game_fake50.npz"))
    data = (g["ptr"], g["idx"], g["val"], int(g["n_items"]))
    a, b = _defender(data, gpu_device), _defender(data, gpu_device)
    sa, sb = a.defense_step(), b.defense_step()
    assert sa == sb and torch.equal(a.distances, b.distances) and torch.equal(a.eigenvectors, b.eigenvectors)
    assert np.array_equal(a.eigenvalues, b.eigenvalues)
    bad = g["val"].copy()
    bad[17] = np.nan
    with pytest.raises(ValueError):
        _defender((g["ptr"], g["idx"], bad, int(g["n_items"])), gpu_device).defense_step()
    bad[17] = np.inf
    with pytest.raises(ValueError):
        _defender((g["ptr"], g["idx"], bad, int(g["n_items"])), gpu_device).defense_step()
    with pytest.raises(RuntimeError, match="residuals"):
        _defender(data, gpu_device, max_iter=1).defense_step()


def test_defense_workflow_with_pca_defender(gpu_device):
    d = synth.make("tiny")
    ds = dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                             device=gpu_device, graph_source="train", seed=5)
    defender = model.from_config("defender", "PCASelectUsers", attack_num=15, device=gpu_device)
    wf = workflow.from_config("defense", victim_data=ds, attack_data=None, victim=model.from_config("victim", "lightgcn", latent_dim_rec=32),
                              attacker=workflow.RandomAttack(ds.n_items, attack_num=15, filler_num=8, seed=3),
                              defender=defender, rec_epoch=2, attack_epoch=0, device=gpu_device)
    res = wf.execute()
    assert wf.defender.user_num == wf.fake_dataset.n_users == ds.n_users + 15
    assert res["n_flagged"] == flag_count(15, ds.n_users + 15)
    assert all(np.isfinite(v) for part in ("attacked", "defended") for v in res[part].values())
