"""GPU tests of the PCASelectUsers defender (csrc/pca.hip + recad_amd/defense): against the reference's own run on
the game data (tests/golden/make_golden_pca.py), fp64 residuals at the ml1m / yelp / config-4 shapes, determinism,
failure modes, the defence workflow, and the solver beyond kVals = 3: the 16-wide block, near-degenerate eigenpairs, explicit
ratings at a middle size and rank-deficient input."""
import os
import time

import numpy as np
import pytest
import torch

from recad_amd import dataset, model, synth, workflow
from recad_amd.defense.pca_select_users import flag_count, sign_fix

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


# ---- beyond kVals = 3: the 16-wide block, eigenpairs close together, rank-deficient input ------------------------------------
#
# Bounds.  res_j is the solver's own residual ||C' v_j - lambda_j v_j|| (defender.residuals) for the operator C' it applies in
# fp32; C' differs from the exact C by the rounding of D^-1 (applied twice, 1.5 * 2^-23 relative each: the bound of
# test_defender_kernels_gpu.py) and of the two fp32 SpMMs (row-wise at most (len + 4) * 2^-24, adding up like a random walk
# over rows a few hundred long): OP_ERR = 16 * 2^-24 * lambda_1 covers both, and is a tenth of the default tol * lambda_1.
#   eigenvalues (Weyl):     |lambda_j - lambda_j(C)| <= res_j + OP_ERR, or rtol 1e-4 (the tolerance of test_against_reference,
#                           which also covers the reference's fp32 ARPACK values) where that is looser
#   eigenvectors (sin-theta theorem): sin(angle) <= (res_j + OP_ERR) / (gap_j - res_j - OP_ERR), gap_j the distance from
#                           lambda_j to its nearest neighbour in the recorded fp64 spectrum.  The tests require
#                           res_j + OP_ERR <= gap_j / 2, which makes that at most C_SIN = 2 times (res_j + OP_ERR) / gap_j.
#                           Added: the reference vector's own error (vecs_err of the fixture: fp32 ARPACK against fp64 eigh)
#                           and 2^-22 for the fp32 storage of the two unit vectors.
#   distances:              dist_u = (a_u o a_u) . sum_j v_j, so |dist_u - ref_u| <= ||a_u o a_u||_2 * sum_j (vector bound j),
#                           plus 2^-22 * (a_u o a_u) . |w| for the fp32 rounding of w and of dist itself.
OP_ERR = 16 * 2.0 ** -24
C_SIN = 2.0


def _load_case(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    base = np.load(os.path.join(GOLDEN, str(g["csr_from"]) + ".npz")) if "csr_from" in g.files else g
    assert int(base["n_users"]) == int(g["n_users"]) and int(base["n_items"]) == int(g["n_items"])
    return g, (base["ptr"], base["idx"], base["val"], int(base["n_items"]))


def _gaps(spectrum, k):
    s = np.asarray(spectrum, dtype=np.float64)
    up = np.concatenate([[np.inf], s[:k - 1] - s[1:k]])
    return np.minimum(up, s[:k] - s[1:k + 1])


def _eig_tol(d, lam_ref):
    return np.maximum(d.residuals + OP_ERR * d.eigenvalues[0], 1e-4 * np.abs(lam_ref))


def _check_eigenpairs(d, spam, g, data, spectrum, vec_err):
    """The defender's result against a fixture's reference run (vals, vecs_conv, dist_conv, spam_conv) through the bounds above;
    vec_err is the reference eigenvectors' own error as the fixture's maker measured it."""
    k, U = d.k, int(g["n_users"])
    lam1 = d.eigenvalues[0]
    err = d.residuals + OP_ERR * lam1
    gap = _gaps(spectrum, k)
    print(f"k {k} iterations {d.iterations} res/lam1 {d.residuals / lam1} err/gap {err / gap}")
    assert np.all(err <= 0.5 * gap), ("the comparison needs residuals below half the eigengap", err / gap)
    assert np.all(np.abs(d.eigenvalues - spectrum[:k]) <= _eig_tol(d, spectrum[:k])), (d.eigenvalues, spectrum[:k])
    assert np.all(np.abs(d.eigenvalues - g["vals"][:k]) <= _eig_tol(d, g["vals"][:k])), (d.eigenvalues, g["vals"])
    bound = C_SIN * err / gap + vec_err[:k] + 2.0 ** -22
    v = d.eigenvectors.cpu().numpy().astype(np.float64)
    r = g["vecs_conv"][:, :k].astype(np.float64)
    v, r = v / np.linalg.norm(v, axis=0), r / np.linalg.norm(r, axis=0)
    diff = np.linalg.norm(v - r, axis=0)          # 2 sin(angle / 2) under the shared sign convention: at most 1.01 sin(angle) here
    print(f"  vector distance / bound {diff / bound}")
    assert np.all(diff <= 1.01 * bound), (diff, bound)
    ptr, idx, val, _ = data
    rows = np.repeat(np.arange(U), np.diff(ptr))
    a2 = val.astype(np.float64) ** 2
    w = np.abs(g["vecs_conv"][:, :k].astype(np.float64).sum(axis=1))
    dbound = np.sqrt(np.bincount(rows, weights=a2 * a2, minlength=U)) * (1.01 * bound).sum() \
        + 2.0 ** -22 * np.bincount(rows, weights=a2 * w[idx], minlength=U)
    dist = d.distances.cpu().numpy().astype(np.float64)
    print(f"  distance error / bound {np.max(np.abs(dist - g['dist_conv']) / np.maximum(dbound, 1e-300))}")
    assert np.all(np.abs(dist - g["dist_conv"]) <= dbound)
    m = flag_count(int(g["attack_num"]), U)
    assert len(spam) == m == len(g["spam_conv"])
    dm = np.sort(g["dist_conv"], kind="stable")[m - 1]
    for u in set(spam) ^ set(g["spam_conv"].tolist()):
        assert abs(g["dist_conv"][u] - dm) <= dbound[u] + dbound.max(), (u, g["dist_conv"][u], dm)
    assert d.predLabels.sum() == m and [u for u, _ in d.disSort[:m]] == spam


@pytest.mark.parametrize("name", ["pca_game_fake50_k8", "pca_dev_k5", "pca_dev_k12"])
def test_against_reference_beyond_k3(gpu_device, name):
    """The reference's own runs at kVals = 8 (game + 50 fakes) and kVals = 5, 12 (dev), default block, tol and max_iter.  dev has
    lambda_5 and lambda_6 0.13 % of lambda_1 apart: at the default tol the residuals are still under 1 % of that gap, so the
    default is kept and the per-vector bound does the rest."""
    g, data = _load_case(name)
    d = _defender(data, gpu_device, kVals=int(g["kVals"]), attack_num=int(g["attack_num"]))
    spam = d.defense_step()
    assert d.k == int(g["k"]) == int(g["kVals"]) and d.eigenvectors.shape == (int(g["n_items"]), d.k)
    _check_eigenpairs(d, spam, g, data, g["spectrum"], g["vecs_err"])


SPECTRA = {"pca_game_fake50": "pca_game_fake50_k8", "pca_dev_kreset": "pca_dev_k5"}


@pytest.mark.parametrize("k", [1, 2, 4, 5, 6, 8, 12, 16])
@pytest.mark.parametrize("name", ["pca_game_fake50", "pca_dev_kreset"])
def test_kvals_sweep_default_configuration(gpu_device, name, k):
    """Every block the default rule picks converges within the default max_iter on both stored matrices (kVals = 5 on dev did
    not with an 8-wide block: DESIGN.md section 9), to fp64 residuals within tol * lambda_1 and the dense fp64 spectrum."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    spectrum = np.load(os.path.join(GOLDEN, SPECTRA[name] + ".npz"))["spectrum"]
    U, I = int(g["n_users"]), int(g["n_items"])
    d = _defender((g["ptr"], g["idx"], g["val"], I), gpu_device, kVals=k, attack_num=50)
    spam = d.defense_step()
    print(f"{name} kVals {k}: {d.iterations} iterations, residuals / lambda_1 {d.residuals / d.eigenvalues[0]}")
    assert d.k == k and len(d.eigenvalues) == k and d.eigenvectors.shape == (I, k) and len(spam) == flag_count(50, U)
    dev = gpu_device
    res, _ = _fp64_residuals(U, I, torch.from_numpy(g["ptr"]).to(dev), torch.from_numpy(g["idx"]).to(dev), torch.from_numpy(g["val"]).to(dev),
                             d.eigenvalues, d.eigenvectors)
    print(f"  fp64 residuals / lambda_1 {res / d.eigenvalues[0]}")
    assert np.all(res <= d.tol * d.eigenvalues[0]), (res / d.eigenvalues[0], d.iterations)
    assert np.all(np.abs(d.eigenvalues - spectrum[:k]) <= _eig_tol(d, spectrum[:k])), (d.eigenvalues, spectrum[:k])
    assert np.all(np.isfinite(d.distances.cpu().numpy()))


def test_kvals_above_the_block_is_refused(gpu_device):
    g = np.load(os.path.join(GOLDEN, "pca_dev_kreset.npz"))
    data = (g["ptr"], g["idx"], g["val"], int(g["n_items"]))
    assert 17 < min(int(g["n_users"]), int(g["n_items"]))
    with pytest.raises(ValueError, match="kVals|block"):
        _defender(data, gpu_device, kVals=17).defense_step()
    with pytest.raises(ValueError, match="kVals"):
        _defender(data, gpu_device, kVals=12, block=8).defense_step()


def test_block16_at_k3_matches_block8(gpu_device):
    """block = 16 forced at kVals = 3 gives the eigenpairs block = 8 gives: each within the bounds of the reference run."""
    g, data = _load_case("pca_game_fake50")
    k8 = np.load(os.path.join(GOLDEN, "pca_game_fake50_k8.npz"))
    spectrum = k8["spectrum"]
    runs = {}
    for b in (8, 16):
        d = _defender(data, gpu_device, kVals=3, attack_num=int(g["attack_num"]), block=b)
        spam = d.defense_step()
        _check_eigenpairs(d, spam, g, data, spectrum, k8["base_vecs_err"])
        runs[b] = d
    assert runs[8].iterations != runs[16].iterations or not torch.equal(runs[8].eigenvectors, runs[16].eigenvectors), "block was ignored"
    assert np.all(np.abs(runs[8].eigenvalues - runs[16].eigenvalues) <= _eig_tol(runs[8], spectrum[:3]) + _eig_tol(runs[16], spectrum[:3]))


_MID = {}


def _mid_matrix(dev):
    """About 6 000 x 3 700 with ratings 1..5: 200 columns every user rated identically (constant: scale 1), empty rows and
    columns, 50 planted fake rows.  Returns the CSR on the device and the dense fp64 spectrum of C (computed once)."""
    if not _MID:
        rng = np.random.default_rng(77)
        U, I, n_const, n_fake = 6000, 3700, 200, 50
        const_cols = np.sort(rng.choice(I, n_const, replace=False))
        const_val = rng.integers(1, 6, n_const).astype(np.float32)
        free = np.setdiff1d(np.arange(I), const_cols)
        empty_cols = set(free[rng.choice(len(free), 40, replace=False)].tolist()) | {int(free[0]), int(free[-1])}
        pool = np.array([c for c in free if c not in empty_cols])
        pop = rng.pareto(1.2, len(pool)) + 0.05
        pop /= pop.sum()
        target = int(pool[np.argmax(pop) - 1])
        bare = set(rng.choice(U - n_fake, 30, replace=False).tolist()) | {0, U - n_fake - 1}      # users with no rating of their own
        rows = []
        for u in range(U):
            if u >= U - n_fake:
                c = np.unique(np.concatenate([[target], rng.choice(pool, 36, replace=False)]))
                v = np.where(c == target, 5.0, np.clip(np.round(rng.normal(3.6, 1.1, len(c))), 1, 5))
            elif u in bare:
                c, v = np.zeros(0, dtype=np.int64), np.zeros(0)
            else:
                c = np.unique(rng.choice(pool, int(rng.integers(5, 60)), p=pop))
                v = np.clip(np.round(rng.normal(3.6, 1.1, len(c))), 1, 5)
            c = np.concatenate([c, const_cols])
            v = np.concatenate([v, const_val])
            o = np.argsort(c, kind="stable")
            rows.append((c[o], v[o]))
        ptr = np.zeros(U + 1, dtype=np.int32)
        ptr[1:] = np.cumsum([len(c) for c, _ in rows])
        idx = np.concatenate([c for c, _ in rows]).astype(np.int32)
        val = np.concatenate([v for _, v in rows]).astype(np.float32)
        rp, col, vv = torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(val).to(dev)
        r = torch.repeat_interleave(torch.arange(U, device=dev), (rp[1:] - rp[:-1]).long())
        A = torch.zeros(U, I, dtype=torch.float64, device=dev)
        A[r, col.long()] = vv.double()
        var = A.var(dim=0, unbiased=False)
        n_unit = int((var.float() < 10 * torch.finfo(torch.float32).eps).sum().item())
        assert n_const + len(empty_cols) <= n_unit < I // 4, n_unit      # the unpopular tail leaves more columns unrated
        var = torch.where(var.float() < 10 * torch.finfo(torch.float32).eps, torch.ones_like(var), var)
        S = A / torch.sqrt(var)
        lam = torch.linalg.eigvalsh(S.t() @ S).flip(0)[:24].cpu().numpy()
        _MID.update(U=U, I=I, rp=rp, col=col, val=vv, lam=lam)
    return _MID


@pytest.mark.parametrize("k", [3, 8])
def test_mid_size_explicit_ratings(gpu_device, k):
    M = _mid_matrix(gpu_device)
    U, I, rp, col, val, lam = (M[key] for key in ("U", "I", "rp", "col", "val", "lam"))
    d = _defender((rp, col, val, I), gpu_device, kVals=k, attack_num=50)
    spam = d.defense_step()
    print(f"mid k {k}: {d.iterations} iterations, lambda {d.eigenvalues}, dense {lam[:k]}")
    assert len(spam) == flag_count(50, U)
    res, _ = _fp64_residuals(U, I, rp, col, val, d.eigenvalues, d.eigenvectors)
    print(f"  residuals / lambda_1: solver {d.residuals / d.eigenvalues[0]} fp64 {res / d.eigenvalues[0]}")
    assert np.all(res <= d.tol * d.eigenvalues[0]), (res / d.eigenvalues[0], d.iterations)
    assert np.all(np.abs(d.eigenvalues - lam[:k]) <= d.residuals + OP_ERR * lam[0]), (d.eigenvalues, lam[:k], d.residuals)


def _dense_eigs(A):
    A = np.asarray(A, dtype=np.float64)
    var = A.var(axis=0)
    var = np.where(var.astype(np.float32) < 10 * np.finfo(np.float32).eps, 1.0, var)
    S = A / np.sqrt(var)
    lam, vec = np.linalg.eigh(S.T @ S)
    return lam[::-1], vec[:, ::-1], S.T @ S


def test_rank_deficient_five_users(gpu_device):
    """5 users x 40 items: C has at most 5 nonzero eigenvalues, fewer than either block width.  kVals = 3 is the dense answer."""
    rng = np.random.default_rng(3)
    A = np.where(rng.random((5, 40)) < 0.6, rng.integers(1, 6, (5, 40)), 0).astype(np.float32)
    lam, vec, C = _dense_eigs(A)
    assert lam[4] > 1e-3 * lam[0] and abs(lam[5]) < 1e-9 * lam[0]
    d = _defender(A, gpu_device, kVals=3, attack_num=2)
    spam = d.defense_step()
    print(f"5 x 40: {d.iterations} iterations, lambda {d.eigenvalues} dense {lam[:3]}")
    assert d.k == 3 and len(spam) == flag_count(2, 5)
    assert np.all(np.abs(d.eigenvalues - lam[:3]) <= d.residuals + OP_ERR * lam[0]), (d.eigenvalues, lam[:3])
    V = d.eigenvectors.cpu().numpy().astype(np.float64)
    res = np.linalg.norm(C @ V - V * d.eigenvalues[None, :], axis=0)
    assert np.all(res <= d.tol * lam[0]), res / lam[0]
    dist = d.distances.cpu().numpy()
    assert np.all(np.isfinite(dist))
    err = d.residuals + OP_ERR * lam[0]
    gap = _gaps(lam, 3)
    assert np.all(err <= 0.5 * gap)
    bound = (1.01 * (C_SIN * err / gap + 2.0 ** -22)).sum()
    want = (A.astype(np.float64) ** 2) @ sign_fix(vec[:, :3]).sum(axis=1)
    assert np.all(np.abs(dist - want) <= np.linalg.norm(A.astype(np.float64) ** 2, axis=1) * bound + 2.0 ** -22 * np.abs(want).max())


def test_every_column_constant(gpu_device):
    """Every user rates every item j with the same value c_j: every variance is 0, every scale 1, and C = U c c^T has one nonzero
    eigenvalue, fewer than kVals = 3.  The call ends in a result (lambda_1 right, the rest ~ 0, finite distances) or in a
    RuntimeError / ValueError that says what happened: never numpy's LinAlgError, never NaN."""
    c = np.array([1, 2, 3, 4, 5] * 4, dtype=np.float32)
    A = np.tile(c, (30, 1))
    lam1 = 30.0 * float((c.astype(np.float64) ** 2).sum())
    d = _defender(A, gpu_device, kVals=3, attack_num=3)
    try:
        spam = d.defense_step()
    except (RuntimeError, ValueError) as e:
        assert not isinstance(e, np.linalg.LinAlgError)
        assert "rank" in str(e) or "converge" in str(e), str(e)
        return
    print(f"constant columns: {d.iterations} iterations, lambda {d.eigenvalues}")
    assert abs(d.eigenvalues[0] - lam1) <= 1e-5 * lam1 and np.all(np.abs(d.eigenvalues[1:]) <= 1e-5 * lam1), d.eigenvalues
    assert np.all(np.isfinite(d.distances.cpu().numpy())) and np.all(np.isfinite(d.eigenvectors.cpu().numpy()))
    assert len(spam) == flag_count(3, 30)
