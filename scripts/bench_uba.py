"""UBA budget_matrix() timings (not the driver's bench line): the whole budget x 10 loop of rk_uba_prob -- 60 redraws, score
passes and counts, one read-back -- on the ml1m-shaped synthetic explicit data at the registry defaults (50 target users,
budget 6, selected_ids [62]), in both modes, and once on the CPU restatement (tests/_uba_restate.py, the weighted-sum form; the
reference's own dense (M+N)^2 form does not fit a sitting at this shape).  Wall clock around the synchronous call (it ends in
its read-back), the median of --reps calls after --warmup.  The call is ~240 launches, so the time holds launch gaps as well
as kernel time.  One JSON line, appended to --out (profiles/bench_uba_mi355x.jsonl).

    python scripts/bench_uba.py [--reps 10] [--warmup 2] [--out FILE] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_uba_mi355x.jsonl"))
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from recad_amd import dataset, model, synth
    from tests import _uba_restate as R

    dev = torch.device("cuda:0")
    r = synth.with_ratings("ml1m")
    explicit = dataset.from_config("explicit", "ml1m", train_csr=r["train"], valid_csr=r["valid"], test_csr=r["test"], device=dev)
    res = {"shape": "ml1m", "n_users": int(explicit.n_users), "n_items": int(explicit.n_items), "nnz": int(len(r["train"][1])),
           "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for hops in ("elementwise", "matrix"):
        att = model.from_config("attacker", "uba", seed=3, hops=hops, device=dev).I(dataset=explicit)
        res["n_targets"], res["budget"], res["side_nnz"], res["scratch_bytes"] = len(att.target_user_id), att.budget, int(att.side_ptr[-1]), att.scratch_bytes
        med, lo, hi = _median_ms(att.budget_matrix, a.reps, a.warmup)
        p = att.budget_matrix()
        res[hops] = {"median_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3), "prob_mean": float(p.mean()),
                     "tie_dependent": att.last_tie_dependent}
    if not a.no_cpu:
        ptr, idx, val = (np.asarray(x) for x in r["train"])
        mat = R.dense(explicit.n_users, explicit.n_items, ptr, idx, val)
        draws = np.random.default_rng(3).integers(1, 6, size=(att.budget, R.TRIALS, int(att.side_ptr[-1])))
        t0 = time.perf_counter()
        ref, ties, _, _ = R.prob(mat, att.target_user_id, att._s, att.budget, draws, "matrix")
        res["cpu_restatement_matrix_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        assert np.array_equal(att.replay_budget_matrix(draws), ref) and att.last_tie_dependent == ties
        res["replay_equals_restatement"] = True
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
