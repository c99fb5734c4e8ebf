"""The detection probe of DESIGN.md section 17 on synthetic data: 50 profiles of the project's heuristic attackers, built from
their host restatements (tests/_heuristic_restate.py: the exact filler columns of the device's draw, the popularity rule, the
rounding and clipping of the values; the normal draws themselves come from numpy here), appended to synth.make("ml1m"), scored
by the CatchSync restatement and, for comparison, by DegSim in float64.  scripts/cs_detection_probe.py prints the table."""
import numpy as np

from recad_amd import default, synth
from tests import _catchsync_restate as R
from tests import _heuristic_restate as H

ATTACKERS = ("random", "average", "bandwagon", "segment")
N_FAKE, FILLERS, TARGET, SEED = 50, 36, 1000, 20141


def clean(shape="ml1m"):
    d = synth.make(shape)
    ptr, idx = (np.asarray(a) for a in d["train"])
    U, I = int(d["n_users"]), int(d["n_items"])
    val = np.asarray(synth.with_ratings(d)["train"][2], dtype=np.float64)
    return ptr[: U + 1].astype(np.int64), idx[: ptr[U]].astype(np.int64), val[: ptr[U]], U, I


def fake_ratings(kind, idx, val, n_items):
    """[N_FAKE, I] float32 ratings of one attacker: the target and the selected items at 5, 36 fillers valued as the attacker
    values them."""
    count, mean, gmean, gstd, _ = H.item_stats(n_items, idx, val)
    mode = {"random": H.GLOBAL, "average": H.ITEM, "bandwagon": H.GLOBAL, "segment": H.ONES}[kind]
    selected = []
    if kind == "bandwagon":
        selected = H.popular(count, 11)[0].tolist()
    elif kind == "segment":
        selected = [i for i in default.MODEL["attacker"]["segment"]["selected_ids"] if i < n_items]
    cols = H.draw_cols(SEED, ATTACKERS.index(kind), N_FAKE, FILLERS, n_items, [TARGET] + selected)
    x = None
    if mode != H.ONES:
        mu, sd = H.moments(mode, cols, gmean, gstd, mean, count)
        x = np.random.default_rng(SEED + ATTACKERS.index(kind)).normal(mu, np.abs(sd))
    return H.profiles(N_FAKE, n_items, [TARGET], selected, cols, x)


def poisoned(kind, keep, base=None):
    """(ptr, idx, U_real, I) with the fake rows appended.  keep "all": every rated item of a profile is an edge; "above4": only
    the ratings above 4, what the defence workflow's implicit injection (filter_num = 4) keeps."""
    ptr, idx, val, U, I = base or clean()
    out = fake_ratings(kind, idx, val, I)
    mask = out > (0 if keep == "all" else 4)
    fu, fi = np.nonzero(mask)
    new_ptr = np.concatenate([ptr, ptr[-1] + np.cumsum(np.bincount(fu, minlength=N_FAKE))])
    return new_ptr, np.concatenate([idx, fi]), U, I


def top_hits(scores, U, largest=True):
    """How many of the N_FAKE appended users are among the N_FAKE largest (smallest) scores, ties to the lower id."""
    s = np.asarray(scores, dtype=np.float64)
    order = np.lexsort((np.arange(len(s)), -s if largest else s))[:N_FAKE]
    return int((order >= U).sum())


def catchsync_hits(ptr, idx, U, I, grid_bits, min_items):
    """{score: fakes among the 50 largest}."""
    deg, reach = R.features(ptr, idx, I)
    cell_of, count, info = R.cells(deg, reach, grid_bits)
    pair, back = R.user_sums(ptr, idx, cell_of, count, max(info[0], 1))
    return {m: top_hits(R.scores(ptr, pair, back, info, m, min_items), U) for m in R.MODES}


def degsim_hits(ptr, idx, U, I, k=25):
    """(fakes among the 50 lowest, among the 50 highest) DegSim, float64, implicit values."""
    n = len(ptr) - 1
    A = np.zeros((n, I))
    A[np.repeat(np.arange(n), np.diff(ptr)), idx] = 1.0
    A /= np.sqrt(np.maximum(A.sum(axis=1, keepdims=True), 1.0))
    W = A @ A.T
    np.fill_diagonal(W, -1.0)
    d = np.sort(np.partition(W, n - k, axis=1)[:, n - k:], axis=1).mean(axis=1)
    return top_hits(d, U, largest=False), top_hits(d, U, largest=True)
