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


def golden_case(recad, torch, name, tag, k, attack_num, n_fake):
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
    np.savez_compressed(os.path.join(OUT, f"pca_{tag}.npz"), **out)
    print(tag, {k_: getattr(v, "shape", v) for k_, v in out.items()}, "vals", out["vals"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "recad_golden_scratch"))
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
    golden_case(recad, torch, "game", "game_fake50", 3, 50, 50)
    golden_case(recad, torch, "dev", "dev_kreset", 10 ** 6, 50, 0)


if __name__ == "__main__":
    main()
