#!/usr/bin/env python3
"""Generate tests/golden/heur_game_{average,segment,bandwagon}.npz, the fixtures of the heuristic attackers, by IMPORTING
the reference (gusye1234/recad v0.0.2, a checkout passed as --reference).  Modelled on make_golden_aush.py; run by hand, CPU
only; nothing under tests/ or the product imports it.  It copies no reference source: it drives the reference's own

    recad.dataset.from_config("explicit", "game")
    recad.model.from_config("attacker", "average" | "segment" | "bandwagon", ...).I(dataset=...) / generate_fake

and records every random draw on the way by wrapping np.random.choice (the fillers of a row) and np.random.normal (their
values: one call per filler for average, one call for all of them for bandwagon, none for segment).  The game train / valid /
test rows themselves are stored in aush_game_partial.npz.

Cases (numpy is seeded right before each generate_fake):
  average    a_: the default sizes (attack_num 50, filler_num 36), target [0]
             b_: attack_num 7, filler_num 5, targets [3, 11] -- rate 3, so row 6 rates no target
  segment    selected_ids [62, 7, 300], target [5], default sizes
  bandwagon  selected_ids [] (passed explicitly: the reference's from_config would otherwise read the segment entry,
             heuristic.py:264-266), target [0], default sizes: the 11 most rated items are selected
Every file also holds the statistics of the train ratings as the reference computes them: global_mean / global_std
(heuristic.py:91-92), item_mean [n_items] (heuristic.py:94-97; 0 where item_count is 0), item_count, and popular_ids /
popular_counts, the bandwagon attacker's 11 selected items in its order with their counts, plus count_12th.
Profiles are stored as (row, col, value) triplets; each file stays well under 1 MB.

Two conditions are asserted here and stated again by the tests: no recorded normal value lies within 2^-20 of a half-integer
(so np.round of it is decidable by any float64 restatement), and the 11th and 12th largest item counts differ (so the popular
SET is unique; inside it the reference's order among equal counts is an unstable sort's).

Usage:
    python tests/golden/make_golden_heuristic.py --reference PATH [--scratch DIR]
"""
import argparse
import os
import shutil
import sys
import tempfile
import zipfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 2023
HALF_MARGIN = 2.0 ** -20


class Recorder:
    """Wraps np.random.choice and np.random.normal while active."""

    def __init__(self):
        self.choice, self.normal = [], []

    def __enter__(self):
        self.real = (np.random.choice, np.random.normal)
        real_choice, real_normal = self.real

        def choice(*a, **kw):
            out = real_choice(*a, **kw)
            self.choice.append(np.asarray(out).copy())
            return out

        def normal(*a, **kw):
            out = real_normal(*a, **kw)
            self.normal.append(np.asarray(out, dtype=np.float64).reshape(-1).copy())
            return out

        np.random.choice, np.random.normal = choice, normal
        return self

    def __exit__(self, *exc):
        np.random.choice, np.random.normal = self.real


def run_case(att, targets, seed, prefix=""):
    np.random.seed(seed)
    with Recorder() as rec:
        fake = att.generate_fake(target_id_list=list(targets))
    n, F = att.attack_num, att.filler_num
    assert len(rec.choice) == n
    cols = np.stack(rec.choice).astype(np.int32)
    assert cols.shape == (n, F)
    nz = np.nonzero(fake)
    out = {"attack_num": np.int64(n), "filler_num": np.int64(F), "targets": np.asarray(targets, dtype=np.int64), "seed": np.int64(seed),
           "selected_ids": np.asarray(getattr(att, "selected_ids", []), dtype=np.int64), "cols": cols,
           "fake_rows": nz[0].astype(np.int32), "fake_cols": nz[1].astype(np.int32), "fake_vals": fake[nz].astype(np.float32),
           "fake_shape": np.asarray(fake.shape, dtype=np.int64)}
    if rec.normal:
        vals = np.concatenate(rec.normal)
        assert vals.shape == (n * F,)
        frac = np.abs(vals - np.floor(vals) - 0.5)
        assert frac.min() > HALF_MARGIN, f"a normal draw within 2^-20 of a half-integer (seed {seed}): choose another seed"
        out["vals"] = vals.reshape(n, F)
    return {prefix + k: v for k, v in out.items()}


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
    kvr = ds.info_describe()["train_kvr"]
    I = int(ds.info_describe()["n_items"])

    def attacker(name, **kw):
        return recad.model.from_config("attacker", name, **kw).I(dataset=ds)

    avg = attacker("average")
    band = attacker("bandwagon", selected_ids=[])
    count = np.bincount(kvr[:, 1].astype(np.int64), minlength=I)
    mean = np.zeros(I, dtype=np.float64)
    for iid, m in avg.item_mean_dict.items():
        mean[int(iid)] = m
    assert set(int(i) for i in avg.item_mean_dict) == set(np.nonzero(count)[0].tolist())
    top = np.sort(count)[::-1]
    assert top[10] != top[11], "the 11th and 12th largest item counts are equal: the popular set is not unique"
    popular = np.asarray(band.selected_ids, dtype=np.int64)
    stats = {"n_users": np.int64(ds.info_describe()["n_users"]), "n_items": np.int64(I), "n_ratings": np.int64(len(kvr)),
             "global_mean": np.float64(avg.global_mean), "global_std": np.float64(avg.global_std), "item_mean": mean,
             "item_count": count.astype(np.int64), "popular_ids": popular, "popular_counts": count[popular].astype(np.int64),
             "count_12th": np.int64(top[11]), "max_rating": np.float64(np.abs(kvr[:, 2]).max())}
    assert float(band.global_mean) == float(avg.global_mean) and float(band.global_std) == float(avg.global_std)

    a = run_case(avg, [0], SEED, "a_")
    a.update(run_case(attacker("average", attack_num=7, filler_num=5), [3, 11], SEED + 1, "b_"))
    np.savez_compressed(os.path.join(OUT, "heur_game_average.npz"), **stats, **a)
    s = run_case(attacker("segment", selected_ids=[62, 7, 300]), [5], SEED + 2)
    np.savez_compressed(os.path.join(OUT, "heur_game_segment.npz"), **stats, **s)
    b = run_case(band, [0], SEED + 3)
    np.savez_compressed(os.path.join(OUT, "heur_game_bandwagon.npz"), **stats, **b)
    for name in ("average", "segment", "bandwagon"):
        p = os.path.join(OUT, f"heur_game_{name}.npz")
        assert os.path.getsize(p) < 1 << 20
        print(name, os.path.getsize(p), "bytes")
    print("mean", stats["global_mean"], "std", stats["global_std"], "popular", popular.tolist(), stats["popular_counts"].tolist(),
          "12th", int(top[11]))
    shutil.rmtree(os.path.join(args.scratch, "generated"), ignore_errors=True)


if __name__ == "__main__":
    main()
