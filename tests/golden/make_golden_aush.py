#!/usr/bin/env python3
"""Generate tests/golden/aush_*.npz, the fixtures of the AUSH attacker and the explicit dataset, by IMPORTING the
reference (gusye1234/recad v0.0.2, a checkout passed as --reference).  Modelled on make_golden_pca.py; run by hand,
CPU only; nothing under tests/ or the product imports it.  It copies no reference source: it drives the reference's own

    recad.dataset.from_config("explicit", "game") / .partial_sample(user_ratio=0.2)
    recad.model.from_config("attacker", "aush", ...).I(dataset=...) / train_step / generate_fake

and records every random draw on the way by wrapping np.random.choice (sample_fillers, aush.py:60-77),
np.random.shuffle (the ZR pool, aush.py:116), np.random.permutation / np.random.randint (explicit.py:189,
aush.py:181-182) and the dataset's generate_batch (the batch users), plus the loss modules and a forward hook on netG.

Cases (all on the game data, torch.manual_seed(SEED) right before .I(), so the initial weights are reproducible):
  aush_game_f12      filler_num 12, selected_ids [62], target [0], two epochs
  aush_game_s3t2     filler_num 12, selected_ids [62, 7, 300], targets [0, 5], one epoch
  aush_game_fake36   generate_fake at the default filler_num 36, target [0]
  aush_game_partial  partial_sample(user_ratio=0.2) after np.random.seed(PARTIAL_SEED): the kept users / remap

Recorded per training case: a fingerprint of the train rating CSR (the CSR itself is rebuilt from the game kvr rows
stored in aush_game_partial), fingerprints of the initial weights (sum and sum of squares per tensor, float64), per
batch the users, the filler draws [B, filler_num] and the ZR ones [B, |S|] (selected ids ascending), the four losses;
D after each epoch: the ids of the first-layer columns that changed with each one's (sum, L2 norm), the biases in full,
the 150 x 150 layers in full after the last epoch and as per-row (sum, L2 norm) before it, and after the last epoch
the changed first-layer columns of the selected ids plus a seeded sample of W1_SAMPLE others in full; the epoch means;
G after training (its fingerprints).  Each file stays well under 1 MB.

Usage:
    python tests/golden/make_golden_aush.py --reference PATH [--scratch DIR]
"""
import argparse
import math
import os
import shutil
import sys
import tempfile
import zipfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 2023
PARTIAL_SEED = 11
W1_SAMPLE = 256


def fingerprints(state):
    keys = sorted(state)
    out = np.zeros((len(keys), 2), dtype=np.float64)
    for k, name in enumerate(keys):
        a = state[name].detach().double().numpy()
        out[k] = a.sum(), (a * a).sum()
    return np.asarray(keys), out


def csr_fingerprint(ptr, idx, val):
    """[nnz, sum of row pointers, sum of item ids, sum of ratings] of a rating CSR: the training fixtures name the train
    CSR they ran on this way (the CSR itself is rebuilt from the kvr rows stored in aush_game_partial)."""
    return np.asarray([len(idx), ptr.astype(np.float64).sum(), idx.astype(np.float64).sum(), val.astype(np.float64).sum()])


def rating_csr(mat):
    mat = np.asarray(mat, dtype=np.float32)
    nz = mat != 0
    ptr = np.zeros(mat.shape[0] + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(nz.sum(axis=1))
    return ptr, np.nonzero(nz)[1].astype(np.int32), mat[nz]


class Recorder:
    """Wraps the reference's random calls and loss modules while active."""

    def __init__(self, recad, torch, mod, zr_ratio):
        self.recad, self.torch, self.mod, self.zr_ratio = recad, torch, mod, zr_ratio
        self.choice, self.shuffle, self.perm, self.randint = [], [], [], []
        self.bce, self.mse = [], []

    def __enter__(self):
        np_r = np.random
        self.real = (np_r.choice, np_r.shuffle, np_r.permutation, np_r.randint)
        real_choice, real_shuffle, real_perm, real_randint = self.real

        def choice(*a, **kw):
            out = real_choice(*a, **kw)
            self.choice.append(np.asarray(out).copy())
            return out

        def shuffle(x):
            real_shuffle(x)
            self.shuffle.append(np.asarray(x).copy())

        def permutation(x):
            out = real_perm(x)
            self.perm.append(np.asarray(out).copy())
            return out

        def randint(*a, **kw):
            out = real_randint(*a, **kw)
            self.randint.append(np.asarray(out).copy())
            return out

        np_r.choice, np_r.shuffle, np_r.permutation, np_r.randint = choice, shuffle, permutation, randint
        torch_nn = self.torch.nn
        rec = self

        class Shim:
            def __getattr__(self, name):
                return getattr(torch_nn, name)

            @staticmethod
            def BCELoss():
                f = torch_nn.BCELoss()

                def call(x, y):
                    v = f(x, y)
                    rec.bce.append(v.detach().clone())
                    return v
                return call

            @staticmethod
            def MSELoss():
                f = torch_nn.MSELoss()

                def call(x, y):
                    v = f(x, y)
                    rec.mse.append(v.detach().clone())
                    return v
                return call

        self.real_nn = self.mod.nn
        self.mod.nn = Shim()
        return self

    def __exit__(self, *exc):
        np.random.choice, np.random.shuffle, np.random.permutation, np.random.randint = self.real
        self.mod.nn = self.real_nn


def train_case(recad, torch, ds, tag, filler_num, selected_ids, targets, epochs):
    import recad.model.attacker  # noqa: F401

    mod = sys.modules["recad.model.attacker.aush"]
    S = sorted(selected_ids)
    torch.manual_seed(SEED)
    att = recad.model.from_config("attacker", "aush", filler_num=filler_num, selected_ids=list(selected_ids)).I(dataset=ds)
    g0 = {k: v.clone() for k, v in att.netG.state_dict().items()}
    d0 = {k: v.clone() for k, v in att.netD.state_dict().items()}
    out = {"csr_fp": csr_fingerprint(*rating_csr(ds.train_mat)), "n_users": np.int64(ds.n_users), "n_items": np.int64(ds.n_items),
           "filler_num": np.int64(filler_num), "selected_ids": np.asarray(S, dtype=np.int64), "targets": np.asarray(targets, dtype=np.int64),
           "zr_ratio": np.float64(att.ZR_ratio), "lr_d": np.float64(att.config["lr_d"]), "seed": np.int64(SEED),
           "batch_size": np.int64(ds.config["batch_size"]), "epochs": np.int64(epochs)}
    names, fp = fingerprints(g0)
    out["g_names"], out["g_fp0"] = names, fp
    names, fp = fingerprints(d0)
    out["d_names"], out["d_fp0"] = names, fp
    users_l, draws_l, zr_l, losses_l, ep_of = [], [], [], [], []
    real_gb = ds.generate_batch
    means = []
    for ep in range(epochs):
        batch_users = []

        def gb(**kw):
            for dp in real_gb(**kw):
                batch_users.append(dp["users"].cpu().numpy().copy())
                yield dp

        ds.generate_batch = gb
        try:
            with Recorder(recad, torch, mod, att.ZR_ratio) as rec:
                res = att.train_step(target_id_list=list(targets))
        finally:
            ds.generate_batch = real_gb
        means.append(np.asarray(res, dtype=np.float64))
        nb = len(batch_users)
        assert len(rec.shuffle) == nb and len(rec.bce) == 3 * nb and len(rec.mse) == 2 * nb
        pos = 0
        for b in range(nb):
            u = batch_users[b]
            B = len(u)
            draws = np.stack(rec.choice[pos:pos + B]).astype(np.int32)
            pos += B
            pools = rec.shuffle[b]
            keep = pools[math.floor(len(pools) * (1 - att.ZR_ratio)):]
            zr = np.zeros((B, len(S)), dtype=np.uint8)
            for r, c in keep:
                zr[r, S.index(int(c))] = 1
            d_loss = (0.5 * (rec.bce[3 * b] + rec.bce[3 * b + 1])).item()
            losses = [d_loss, rec.mse[2 * b + 1].item(), rec.mse[2 * b].item(), rec.bce[3 * b + 2].item()]
            users_l.append(u.astype(np.int32))
            draws_l.append(draws)
            zr_l.append(zr)
            losses_l.append(losses)
            ep_of.append(ep)
        assert pos == len(rec.choice)
        sd = att.netD.state_dict()
        w1, w10 = sd["main.0.weight"].numpy(), d0["main.0.weight"].numpy()
        changed = np.nonzero(np.any(w1 != w10, axis=0))[0]
        out[f"d{ep}_w1_items"] = changed.astype(np.int32)
        # every changed first-layer column as (sum, L2 norm) in float64; in full only the selected ids' columns and a
        # seeded sample of W1_SAMPLE others, after the last epoch (the fixture stays well under 1 MB)
        cols = w1[:, changed].astype(np.float64)
        out[f"d{ep}_w1_colfp"] = np.stack([cols.sum(axis=0), np.sqrt((cols * cols).sum(axis=0))], axis=1)
        last = ep == epochs - 1
        if last:
            rest = np.setdiff1d(changed, S)
            pick = np.random.default_rng(SEED).choice(rest, size=min(W1_SAMPLE, len(rest)), replace=False)
            full = np.sort(np.concatenate([np.intersect1d(changed, S), pick]))
            out[f"d{ep}_w1_full_items"] = full.astype(np.int32)
            out[f"d{ep}_w1_full_cols"] = w1[:, full].T.copy()
        for k in ("main.0.bias", "main.2.weight", "main.2.bias", "main.4.weight", "main.4.bias", "main.6.weight", "main.6.bias"):
            a = sd[k].numpy()
            if last or a.ndim == 1:
                out[f"d{ep}_{k}"] = a.copy()
            else:   # the 150 x 150 layers of earlier epochs: per-row (sum, L2 norm)
                a = a.astype(np.float64)
                out[f"d{ep}_{k}_rowfp"] = np.stack([a.sum(axis=1), np.sqrt((a * a).sum(axis=1))], axis=1)
    lens = np.asarray([len(u) for u in users_l], dtype=np.int64)
    out["batch_len"] = lens
    out["batch_epoch"] = np.asarray(ep_of, dtype=np.int64)
    out["users"] = np.concatenate(users_l)
    out["draws"] = np.concatenate(draws_l)
    out["zr"] = np.concatenate(zr_l)
    out["losses"] = np.asarray(losses_l, dtype=np.float64)
    out["epoch_means"] = np.stack(means)
    names, fp = fingerprints(att.netG.state_dict())
    out["g_fp_after"] = fp
    out["g_unchanged"] = np.bool_(all(torch.equal(att.netG.state_dict()[k], g0[k]) for k in g0))
    np.savez_compressed(os.path.join(OUT, f"aush_{tag}.npz"), **out)
    print(tag, "batches", lens.tolist(), "means", out["epoch_means"].tolist(), "G unchanged", bool(out["g_unchanged"]))


def fake_case(recad, torch, ds, tag, targets):
    import recad.model.attacker  # noqa: F401

    mod = sys.modules["recad.model.attacker.aush"]
    torch.manual_seed(SEED)
    att = recad.model.from_config("attacker", "aush").I(dataset=ds)
    S = sorted(att.selected_ids)
    seen = {}
    hook = att.netG.register_forward_hook(lambda m, i, o: seen.__setitem__("gen", o.detach().numpy()[:, S].copy()))
    try:
        with Recorder(recad, torch, mod, att.ZR_ratio) as rec:
            fake = att.generate_fake(target_id_list=list(targets))
    finally:
        hook.remove()
    users = rec.perm[0][rec.randint[0]]
    ptr, idx, val = rating_csr(ds.train_mat)
    nz = np.nonzero(fake)
    out = {"ptr": ptr, "idx": idx, "val": val, "n_users": np.int64(ds.n_users), "n_items": np.int64(ds.n_items),
           "filler_num": np.int64(att.filler_num), "attack_num": np.int64(att.attack_num), "selected_ids": np.asarray(S, dtype=np.int64),
           "targets": np.asarray(targets, dtype=np.int64), "seed": np.int64(SEED), "users": users.astype(np.int32),
           "draws": np.stack(rec.choice).astype(np.int32), "gen": seen["gen"].astype(np.float32),
           "fake_rows": nz[0].astype(np.int32), "fake_cols": nz[1].astype(np.int32), "fake_vals": fake[nz].astype(np.float32),
           "fake_shape": np.asarray(fake.shape, dtype=np.int64), "fake_dtype": np.asarray(str(fake.dtype))}
    np.savez_compressed(os.path.join(OUT, f"aush_{tag}.npz"), **out)
    print(tag, fake.shape, fake.dtype, "users", users[:8])


def partial_case(recad, ds, tag):
    np.random.seed(PARTIAL_SEED)
    p = ds.partial_sample(user_ratio=0.2)
    keys = np.asarray(sorted(p.user_map), dtype=np.int64)
    out = {"train_kvr": ds.train_dict.astype(np.int64), "valid_kvr": ds.valid_dict.astype(np.int64),
           "test_kvr": ds.test_dict.astype(np.int64), "seed": np.int64(PARTIAL_SEED), "user_ratio": np.float64(0.2),
           "kept_users": keys, "kept_ids": np.asarray([p.user_map[k] for k in keys], dtype=np.int64),
           "n_users": np.int64(p.n_users), "n_items": np.int64(p.n_items), "train_interactions": np.int64(p.train_size),
           "valid_interactions": np.int64(p.valid_size), "test_interactions": np.int64(p.test_size),
           "orig_n_users": np.int64(ds.n_users), "orig_n_items": np.int64(ds.n_items)}
    ptr, idx, val = rating_csr(p.train_mat)
    out.update(p_ptr=ptr, p_idx=idx, p_val=val)
    np.savez_compressed(os.path.join(OUT, f"aush_{tag}.npz"), **out)
    print(tag, "kept", len(keys), "n_users", p.n_users, "n_items", p.n_items)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "recad_golden_scratch"))
    args = ap.parse_args()
    ref_root = os.path.abspath(args.reference)
    os.makedirs(os.path.join(args.scratch, "data"), exist_ok=True)
    if not os.path.exists(os.path.join(args.scratch, "data", "game")):
        with zipfile.ZipFile(os.path.join(ref_root, "data", "game.zip")) as z:
            z.extractall(os.path.join(args.scratch, "data"))
    os.chdir(args.scratch)
    sys.path.insert(0, ref_root)
    import torch

    torch.set_num_threads(1)
    import recad

    recad.utils.TQDM = False
    ds = recad.dataset.from_config("explicit", "game")
    np.random.seed(SEED)
    train_case(recad, torch, ds, "game_f12", 12, [62], [0], 2)
    np.random.seed(SEED + 1)
    train_case(recad, torch, ds, "game_s3t2", 12, [62, 7, 300], [0, 5], 1)
    np.random.seed(SEED + 2)
    fake_case(recad, torch, ds, "game_fake36", [0])
    partial_case(recad, ds, "game_partial")
    shutil.rmtree(os.path.join(args.scratch, "generated"), ignore_errors=True)


if __name__ == "__main__":
    main()
