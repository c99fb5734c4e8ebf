#!/usr/bin/env python3
"""Generate tests/golden/uba_dsp.npz and uba_prob_elementwise.npz, the fixtures of the UBA attacker's target-user selection, by
IMPORTING the reference (gusye1234/recad v0.0.2, a checkout passed as --reference).  Modelled on make_golden_aush.py; run by
hand, CPU only; nothing under tests/ or the product imports it.  It copies no reference source: it drives the reference's own

    recad.model.from_config("attacker", "uba", ...).I(dataset=stub) / .DSP() / .budget_matrix()

through a dataset stub whose info_describe() returns a seeded dense train_mat (the reference allocates (M+N)^2 doubles several
times per prob_matrix_compute call and a budget_matrix makes 60 calls, so the data is 96 users x 64 items).

uba_dsp.npz: DSP() with budget_matrix replaced by a given prob_mat [50, 6] -- all ones, eight seeded sparse random ones, one
whose number of non-empty groups differs from attack_num, all zero.  Recorded per case: prob_mat, attack_num, the outcome
("ok" or the exception's class name), the returned user_list.

uba_prob_elementwise.npz: budget_matrix() with 50 target users and budget 6.  random.randint of the reference's module is
wrapped: per prob_matrix_compute call the values drawn are stored in the side layout of tests/_uba_restate.py (per target
user its rated items ascending with selected_ids[0] in its place; the entry there is 5), with the call's position list.  Row
lengths: most under 20 ratings, three near 40, so tie-dependent cases (ten or more other items redrawn to 5) exist but stay
rare; the generator asserts that their share is at most MAX_TIE_SHARE, the cap tests/test_uba_host.py asserts again.

Usage:
    python tests/golden/make_golden_uba.py --reference PATH
"""
import argparse
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 2023
U, I, N_TARGETS, BUDGET, S = 96, 64, 50, 6, 62
MAX_TIE_SHARE = 0.10
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))


class Stub:
    """The part of the reference's explicit dataset UBA's constructor and DSP read."""

    def __init__(self, mat):
        self.train_mat = mat
        self.n_users, self.n_items = mat.shape

    def info_describe(self):
        return {"n_users": self.n_users, "n_items": self.n_items, "train_mat": self.train_mat}


def seeded_matrix(rng):
    mat = np.zeros((U, I), dtype=np.float64)
    targets = rng.choice(U, size=N_TARGETS, replace=False)
    long_rows = set(targets[:3].tolist())
    for u in range(U):
        n = int(rng.integers(36, 42)) if u in long_rows else int(rng.integers(3, 20))
        cols = rng.choice(I, size=n, replace=False)
        mat[u, cols] = rng.integers(1, 6, size=n)
    return mat, targets


def attacker(recad, mat, targets, **kw):
    return recad.model.from_config("attacker", "uba", target_user_ids=[int(t) for t in targets], selected_ids=[S], budget=BUDGET,
                                   **kw).I(dataset=Stub(mat))


def dsp_cases(recad, rng):
    mat, targets = seeded_matrix(rng)
    probs, attack_nums = [np.ones((N_TARGETS, BUDGET))], [50]
    for k in range(8):
        p = rng.integers(1, 11, size=(N_TARGETS, BUDGET)) / 10.0
        keep = rng.random((N_TARGETS, BUDGET)) < 0.5
        if k < 5:                                           # every group non-empty: the walk back can start at group attack_num
            keep[np.arange(N_TARGETS), rng.integers(0, BUDGET, size=N_TARGETS)] = True
        probs.append(p * keep)
        attack_nums.append(50)
    p = probs[1].copy()
    p[40:] = 0                                              # 40 non-empty groups at the most, attack_num 50
    probs.append(p)
    attack_nums.append(50)
    probs.append(probs[2].copy())                           # attack_num below the number of groups
    attack_nums.append(30)
    probs.append(np.zeros((N_TARGETS, BUDGET)))
    attack_nums.append(50)
    outcome, lists = [], []
    for p, a in zip(probs, attack_nums):
        att = attacker(recad, mat.copy(), targets, attack_num=a)
        att.budget_matrix = lambda p=p: p.copy()
        try:
            lists.append([int(u) for u in att.DSP()])
            outcome.append("ok")
        except Exception as e:                              # noqa: BLE001 -- the class name is the record
            lists.append([])
            outcome.append(type(e).__name__)
    users = np.full((len(lists), 128), -1, dtype=np.int64)
    for k, l in enumerate(lists):
        users[k, :len(l)] = l
    np.savez_compressed(os.path.join(OUT, "uba_dsp.npz"), prob=np.stack(probs), attack_num=np.asarray(attack_nums, dtype=np.int64),
                        outcome=np.asarray(outcome), n_users_out=np.asarray([len(l) for l in lists], dtype=np.int64), users=users,
                        target_user_ids=targets.astype(np.int64))
    print("uba_dsp", list(zip(outcome, [len(l) for l in lists])))


def prob_case(recad, rng):
    from tests import _uba_restate as R

    mod = sys.modules["recad.model.attacker.uba"]
    mat, targets = seeded_matrix(rng)
    side_ptr, side_col = R.side_layout(mat, targets, S)
    att = attacker(recad, mat.copy(), targets)
    real_random, real_compute = mod.random, att.prob_matrix_compute
    drawn, calls = [], []

    class Shim:
        @staticmethod
        def randint(a, b):
            v = real_random.randint(a, b)
            drawn.append(v)
            return v

    def compute(add_num):
        rated = [np.nonzero(att.train_data_array[u])[0] for u in targets]        # the items this call redraws, in its order
        del drawn[:]
        pos = real_compute(add_num)
        assert len(drawn) == sum(len(r) for r in rated)
        vals = np.full(side_ptr[-1], 5, dtype=np.int8)
        k = 0
        for t, r in enumerate(rated):
            row = side_col[side_ptr[t]:side_ptr[t + 1]]
            at = np.searchsorted(row, r)
            assert np.array_equal(row[at], r)
            vals[side_ptr[t] + at] = drawn[k:k + len(r)]
            k += len(r)
        vals[side_col == S] = 5
        calls.append((add_num, vals, np.asarray(pos, dtype=np.int8)))
        return pos

    mod.random = Shim()
    att.prob_matrix_compute = compute
    real_random.seed(SEED)
    try:
        prob = att.budget_matrix()
    finally:
        mod.random = real_random
    assert [c[0] for c in calls] == [b for b in range(1, BUDGET + 1) for _ in range(R.TRIALS)]
    draws = np.stack([c[1] for c in calls]).reshape(BUDGET, R.TRIALS, -1)
    positions = np.stack([c[2] for c in calls]).reshape(BUDGET, R.TRIALS, N_TARGETS)
    _, n_tie, hits, ties = R.prob(mat, targets, S, BUDGET, draws, "elementwise")
    share = n_tie / ties.size
    assert 0 < share <= MAX_TIE_SHARE, share
    assert np.array_equal((positions != 0)[~ties], hits[~ties])
    np.savez_compressed(os.path.join(OUT, "uba_prob_elementwise.npz"), train_mat=mat.astype(np.int8), target_user_ids=targets.astype(np.int64),
                        selected_id=np.int64(S), budget=np.int64(BUDGET), draws=draws, positions=positions, prob_mat=prob,
                        train_mat_after=att.train_data_array.astype(np.int8), seed=np.int64(SEED))
    print("uba_prob_elementwise", "tie-dependent", n_tie, "of", ties.size, "misses", int((positions == 0).sum()),
          "first target row overwritten", not np.array_equal(att.train_data_array, mat))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    import torch

    torch.set_num_threads(1)
    import recad
    import recad.model.attacker  # noqa: F401

    dsp_cases(recad, np.random.default_rng(SEED))
    prob_case(recad, np.random.default_rng(SEED + 1))


if __name__ == "__main__":
    main()
