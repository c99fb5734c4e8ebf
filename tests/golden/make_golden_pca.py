#!/usr/bin/env python3
"""Generate tests/golden/pca_*.npz, the fixtures of the PCASelectUsers defender, by IMPORTING the reference
(gusye1234/recad v0.0.2, a checkout passed as --reference).  Modelled on make_golden.py; run by hand on a machine
with a checkout of the reference, CPU only; nothing under tests/ or the product imports it.  It copies no reference
source: it drives the reference's own objects

    recad.dataset.from_config("explicit", ...) / recad.model.from_config("defender", "PCASelectUsers", ...)
    defender.defense_step()

with ``torch.zeros(..., device='cuda')`` redirected to the CPU (PCASelectUsers.py:49 allocates its dense array on
the GPU) and ``scipy.sparse.linalg.eigs`` wrapped to record what ARPACK returned.

Cases:
  pca_game_fake50  the explicit game data with 50 seeded fake rating rows appended (ids U..U+49), kVals = 3
  pca_dev_kreset   the explicit dev data, kVals = 10**6: the k >= min(U, I) rule resets k to 3
  pca_game_fake50_k8        the matrix of pca_game_fake50 at kVals = 8 (a 16-wide block in the product)
  pca_dev_k5, pca_dev_k12   the matrix of pca_dev_kreset at kVals = 5 and 12
  pca_sklearn_scale         a small float32 matrix with constant and near-constant columns through
                            sklearn.preprocessing.scale(csr, axis=0, with_mean=False): the scaled values

The k8 / k5 / k12 files do not repeat the rating CSR: `csr_from` names the file that holds it (the maker asserts that the
same seed gave the same matrix).  They add `spectrum`, the 24 largest eigenvalues of C from a dense fp64 eigh, and
`vecs_err`, the sine of the angle between each reference eigenvector (fp32 ARPACK) and the fp64 one: the reference's own
error, which a test adds to its bound (`base_vecs_err`: the same for the vecs_conv stored in `csr_from`).

Each file holds the rating CSR the defender saw (ptr, idx, val, n_users, n_items), the raw run (vals / vecs sorted by
descending eigenvalue, dist, spam) and a second run in which the eigs wrapper applies the project's sign convention
(every eigenvector's entry of largest magnitude positive, lowest index on a tie) before the reference's own code
continues: *_conv arrays.

Usage:
    python tests/golden/make_golden_pca.py --reference PATH [--scratch DIR]
"""
import argparse
import os
import shutil
import sys
import tempfile
import zipfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))


def sign_convention(vecs):
    pos = np.argmax(np.abs(vecs), axis=0)
    s = np.sign(vecs[pos, np.arange(vecs.shape[1])])
    return vecs * np.where(s == 0, 1, s)


def fake_rows(n_items, n_fake, seed, target=0, filler=36):
    """Seeded fake rating rows (user offset, item, rating): the target rated 5, `filler` other items rated
    round(N(3.6, 1.1)) clipped to [1, 5] (the random attack's profile shape)."""
    rng = np.random.default_rng(seed)
    rows = []
    pool = np.setdiff1d(np.arange(n_items), [target])
    for r in range(n_fake):
        rows.append((r, target, 5.0))
        cols = rng.choice(pool, size=filler, replace=False)
        vals = np.clip(np.round(rng.normal(3.6, 1.1, filler)), 1, 5)
        rows.extend((r, int(c), float(v)) for c, v in zip(cols, vals))
    return np.asarray(rows, dtype=np.float64)


def run_defender(recad, torch, ds, k, attack_num, convention):
    import scipy.sparse.linalg as sla

    import recad.model.defense  # noqa: F401

    mod = sys.modules["recad.model.defense.PCASelectUsers"]

    seen = {}
    real_eigs = sla.eigs

    def eigs(*a, **kw):
        vals, vecs = real_eigs(*a, **kw)
        if convention:
            vecs = sign_convention(np.real(vecs)).astype(np.real(vecs).dtype)
        seen["vals"], seen["vecs"] = vals, vecs
        return vals, vecs

    real_zeros = torch.zeros

    def zeros(*a, **kw):
        kw.pop("device", None)
        return real_zeros(*a, **kw)

    mod.scipy.sparse.linalg.eigs = eigs
    torch.zeros = zeros
    try:
        np.random.seed(2023)
        d = recad.model.from_config("defender", "PCASelectUsers", kVals=k, attack_num=attack_num).I(dataset=ds)
        spam = d.defense_step()
    finally:
        mod.scipy.sparse.linalg.eigs = real_eigs
        torch.zeros = real_zeros
    order = np.argsort(-np.real(seen["vals"]), kind="stable")
    dist = np.zeros(len(d.disSort), dtype=np.float64)
    for u, v in d.disSort:
        dist[u] = v
    return {"vals": np.real(seen["vals"])[order].astype(np.float64), "vecs": np.real(seen["vecs"])[:, order].astype(np.float32),
            "dist": dist, "spam": np.asarray(spam, dtype=np.int64), "k": np.int64(d.k)}


def dense_spectrum(mat, vecs_conv, n_lead=24):
    """The n_lead largest eigenvalues of C = S^T S in fp64 (S: columns over their population standard deviation, a variance
    below 10 * FLT_EPSILON in fp32 counting as constant), and the sine of the angle between each column of vecs_conv and the
    fp64 eigenvector of the same rank."""
    A = np.asarray(mat, dtype=np.float64)
    var = A.var(axis=0)
    var = np.where(var.astype(np.float32) < 10 * np.finfo(np.float32).eps, 1.0, var)
    S = A / np.sqrt(var)
    lam, vec = np.linalg.eigh(S.T @ S)
    lam, vec = lam[::-1], vec[:, ::-1]
    err = []
    for j in range(vecs_conv.shape[1]):
        v = vecs_conv[:, j].astype(np.float64)
        v /= np.linalg.norm(v)
        e = vec[:, j] * np.sign(vec[:, j] @ v)
        err.append(np.linalg.norm(v - e))
    return lam[:n_lead].copy(), np.asarray(err), vec


def golden_case(recad, torch, name, tag, k, attack_num, n_fake, csr_from=None):
    ds = recad.dataset.from_config("explicit", name)
    U, I = ds.n_users, ds.n_items
    if n_fake:
        fk = fake_rows(I, n_fake, seed=7)
        fk[:, 0] += U
        ds = recad.dataset.from_config("explicit", name, train_dict=np.concatenate([ds.train_dict.astype(np.float64), fk]),
                                       valid_dict=ds.valid_dict, test_dict=ds.test_dict)
    mat = np.asarray(ds.train_mat, dtype=np.float32)
    nz = mat != 0
    ptr = np.zeros(mat.shape[0] + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(nz.sum(axis=1))
    out = {"ptr": ptr.astype(np.int32), "idx": np.nonzero(nz)[1].astype(np.int32), "val": mat[nz].astype(np.float32),
           "n_users": np.int64(mat.shape[0]), "n_items": np.int64(mat.shape[1]), "kVals": np.int64(k),
           "attack_num": np.int64(attack_num), "n_fake": np.int64(n_fake)}
    for conv in (False, True):
        r = run_defender(recad, torch, ds, k, attack_num, conv)
        for key, v in r.items():
            out[key + ("_conv" if conv else "")] = v
    if csr_from is not None:
        base = np.load(os.path.join(OUT, f"{csr_from}.npz"))
        for key in ("ptr", "idx", "val", "n_users", "n_items"):
            assert np.array_equal(base[key], out[key]), (csr_from, key)
        for key in ("ptr", "idx", "val", "vecs", "dist", "spam", "vals"):      # the matrix is in csr_from; the tests use the *_conv run
            del out[key]
        out["csr_from"] = np.asarray(csr_from)
        out["spectrum"], out["vecs_err"], vec64 = dense_spectrum(mat, out["vecs_conv"])
        b = base["vecs_conv"].astype(np.float64) / np.linalg.norm(base["vecs_conv"].astype(np.float64), axis=0)
        out["base_vecs_err"] = np.asarray([np.linalg.norm(b[:, j] - vec64[:, j] * np.sign(vec64[:, j] @ b[:, j])) for j in range(b.shape[1])])
        out["vals"] = out.pop("vals_conv")
    np.savez_compressed(os.path.join(OUT, f"pca_{tag}.npz"), **out)
    print(tag, {k_: getattr(v, "shape", v) for k_, v in out.items()}, "vals", out["vals"])


def sklearn_scale_case():
    """A 40 x 24 float32 matrix through sklearn's own scale(): columns that are empty, rated identically by every user,
    near-constant (variance below and just above 10 * FLT_EPSILON) and ordinary 1..5 ratings."""
    import scipy.sparse as sp
    from sklearn.preprocessing import scale

    rng = np.random.default_rng(41)
    U, I = 40, 24
    A = np.zeros((U, I), dtype=np.float32)
    for j in range(8, I):
        rows = rng.choice(U, size=int(rng.integers(2, U)), replace=False)
        A[rows, j] = rng.integers(1, 6, len(rows))
    A[:, 1] = 3.0                                  # every user, one value: variance 0
    A[:, 2] = -1.5
    A[:, 3] = 2.0
    A[5, 3] = np.float32(2.0) + np.float32(2.0 ** -10)    # variance 2.3e-8: below the threshold
    A[:, 4] = 2.0
    A[5, 4] = np.float32(2.0) + np.float32(2.0 ** -6)     # variance 5.9e-6: above it
    A[7, 5] = 1e-3                                 # one tiny rating: variance 2.4e-8
    A[7, 6] = 0.05                                 # variance 6.1e-5
    A[3, 7], A[30, 7] = 4.0, 5.0
    csr = sp.csr_matrix(A)
    csr.sort_indices()
    scaled = scale(csr, axis=0, with_mean=False).tocsr()      # scale() answers in CSC
    scaled.sort_indices()
    assert np.array_equal(scaled.indices, csr.indices) and np.array_equal(scaled.indptr, csr.indptr) and scaled.dtype == np.float32
    ratio = scaled.data / csr.data
    unit = np.array([j for j in range(I) if np.any(csr.indices == j) and np.all(ratio[csr.indices == j] == 1.0)], dtype=np.int32)
    assert set(unit.tolist()) == {1, 2, 3, 5}, unit
    np.savez_compressed(os.path.join(OUT, "pca_sklearn_scale.npz"), ptr=csr.indptr.astype(np.int32), idx=csr.indices.astype(np.int32),
                        val=csr.data.astype(np.float32), scaled=scaled.data.astype(np.float32), unit_columns=unit,
                        n_users=np.int64(U), n_items=np.int64(I))
    print("sklearn_scale", csr.nnz, "entries, unscaled columns", unit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "recad_golden_scratch"))
    ap.add_argument("--cases", nargs="*", default=None, help="tags to (re)generate; default: all")
    args = ap.parse_args()
    ref_root = os.path.abspath(args.reference)
    os.makedirs(os.path.join(args.scratch, "data"), exist_ok=True)
    if not os.path.exists(os.path.join(args.scratch, "data", "dev")):
        shutil.copytree(os.path.join(ref_root, "data", "dev"), os.path.join(args.scratch, "data", "dev"))
    if not os.path.exists(os.path.join(args.scratch, "data", "game")):
        with zipfile.ZipFile(os.path.join(ref_root, "data", "game.zip")) as z:
            z.extractall(os.path.join(args.scratch, "data"))
    os.chdir(args.scratch)
    sys.path.insert(0, ref_root)
    import torch

    torch.set_num_threads(1)
    import recad

    recad.utils.TQDM = False
    cases = [("game", "game_fake50", 3, 50, 50, None), ("dev", "dev_kreset", 10 ** 6, 50, 0, None),
             ("game", "game_fake50_k8", 8, 50, 50, "pca_game_fake50"), ("dev", "dev_k5", 5, 50, 0, "pca_dev_kreset"),
             ("dev", "dev_k12", 12, 50, 0, "pca_dev_kreset")]
    for case in cases:
        if args.cases is None or case[1] in args.cases:
            golden_case(recad, torch, *case)
    if args.cases is None or "sklearn_scale" in args.cases:
        sklearn_scale_case()


if __name__ == "__main__":
    main()
