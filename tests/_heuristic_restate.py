"""numpy float64 restatement of csrc/heuristic.hip (rk_heur_item_stats, rk_heur_popular, rk_heur_generate with its replay
form), written from the reference's behaviour (recad/model/attacker/heuristic.py:85-325) and the header's contract.  The
integer side of the device RNG (rk_mix64, the draw keys, Floyd's subset draw, the pool-position-to-item map) is restated
exactly, so the filler COLUMNS of an own-draw run can be compared to the bit; the normal values go through the device's log
and cospi and are only compared in distribution."""
import math

import numpy as np

GLOBAL, ITEM, ONES = 0, 1, 2
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- statistics (heuristic.py:91-98)
def item_stats(n_items, col, val):
    """(item_count, item_mean, global_mean, global_std, n_rated); {0, 0} for the global pair without ratings."""
    col = np.asarray(col, dtype=np.int64)
    v = np.asarray(val, dtype=np.float64)
    count = np.bincount(col, minlength=n_items).astype(np.int64)
    s = np.bincount(col, weights=v, minlength=n_items)
    mean = np.where(count > 0, s / np.maximum(count, 1), 0.0)
    if len(v) == 0:
        return count, mean, 0.0, 0.0, 0
    return count, mean, float(np.mean(v)), float(np.std(v)), int((count > 0).sum())


def item_std(n_items, col, val):
    """Population std per item: what item_std_dict would hold if heuristic.py:98 were np.std (the WRONG variant's scale)."""
    col = np.asarray(col, dtype=np.int64)
    v = np.asarray(val, dtype=np.float64)
    count, mean, _, _, _ = item_stats(n_items, col, val)
    ss = np.bincount(col, weights=(v - mean[col]) ** 2, minlength=n_items)
    return np.sqrt(np.where(count > 0, ss / np.maximum(count, 1), 0.0))


def stat_bound(count, max_abs):
    """|sum of `count` float64 terms of size <= max_abs, in ANY order, minus the exact sum| <= (count - 1) 2^-53 count max_abs
    to first order; divided by count for a mean that is below count * 2^-52 * max_abs, the bound the tests use for the means.
    The same figure serves for the standard deviation: its worst case is max_abs / (2 std) times the mean's (d std = d var /
    (2 std), deviations below max_abs), and a worst case is ~count times what any real summation order loses."""
    return np.asarray(count, dtype=np.float64) * 2.0 ** -52 * max_abs


# ---------------------------------------------------------------- popularity (heuristic.py:252-259)
def popular(count, k):
    """The k most rated items, most rated first, the larger id first among equal counts; never an unrated one."""
    count = np.asarray(count, dtype=np.int64)
    ids = np.nonzero(count > 0)[0]
    order = sorted(ids.tolist(), key=lambda i: (-int(count[i]), -i))[:k]
    return np.asarray(order, dtype=np.int64), count[order] if order else np.zeros(0, dtype=np.int64)


# ---------------------------------------------------------------- profiles (heuristic.py:115-151, 191-220, 274-311)
def moments(mode, cols, gmean, gstd, mean, count, variant=None, std=None):
    """(loc, scale) of every filler's normal value.  variant "true_std": a rated item's scale is its std (not the reference)."""
    cols = np.asarray(cols, dtype=np.int64)
    mu = np.full(cols.shape, gmean, dtype=np.float64)
    sd = np.full(cols.shape, gstd, dtype=np.float64)
    if mode == ITEM:
        rated = np.asarray(count)[cols] > 0
        mu = np.where(rated, np.asarray(mean)[cols], mu)
        sd = np.where(rated, (std if variant == "true_std" else np.asarray(mean))[cols], sd)
    return mu, sd


def profiles(n_rows, n_items, targets, selected, cols, x, variant=None):
    """out [n_rows, n_items] float32: 5 at row r's target (rate = n_rows // len(targets); row r < rate * len(targets) has
    target r // rate, the others none), 5 at every selected id, and at cols[r, k] the value x[r, k] rounded half to even and
    clipped to [1, 5] (x None: the value 1).  variant "mod_targets": row r rates target r % len(targets) (not the reference)."""
    out = np.zeros((n_rows, n_items), dtype=np.float64)
    T = len(targets)
    rate = n_rows // T
    for r in range(n_rows):
        if variant == "mod_targets":
            out[r, targets[r % T]] = 5
        elif rate > 0 and r < rate * T:
            out[r, targets[r // rate]] = 5
    if len(selected):
        out[:, np.asarray(selected, dtype=np.int64)] = 5
    cols = np.asarray(cols, dtype=np.int64)
    v = np.ones(cols.shape) if x is None else np.clip(np.round(np.asarray(x, dtype=np.float64)), 1, 5)
    out[np.arange(n_rows)[:, None], cols] = v
    return out.astype(np.float32)


def value_probs(mu, sd):
    """P(value = 1..5) of clip(round(N(mu, sd)), 1, 5): the normal CDF over the rounding bins (-inf, 1.5], (1.5, 2.5], ...,
    (4.5, inf) -- a boundary has measure zero, so half-to-even does not matter."""
    if sd == 0:
        p = np.zeros(5)
        p[int(np.clip(np.round(mu), 1, 5)) - 1] = 1.0
        return p
    cdf = [0.5 * (1.0 + math.erf((b - mu) / (sd * math.sqrt(2.0)))) for b in (1.5, 2.5, 3.5, 4.5)]
    return np.diff(np.asarray([0.0] + cdf + [1.0]))


# ---------------------------------------------------------------- the device RNG's integer side
def mix64(z):
    z = (np.asarray(z, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw_key(seed, stream, rows, draw):
    with np.errstate(over="ignore"):
        inner = mix64((np.asarray(rows, dtype=np.uint64) << np.uint64(20)) ^ np.uint64(draw))
        return mix64(np.uint64(seed & M64) ^ mix64(np.uint64(stream & M64) ^ inner))


def draw_cols(seed, stream, n_rows, F, n_items, excl):
    """The filler columns of an own-draw run, [n_rows, F] in draw order: Floyd's subset draw over the P = n_items - |excl|
    pool positions (for j = P - F .. P - 1: x uniform in [0, j] from the key's high 32 bits; x, or j when x is taken), then
    position -> item by stepping over the excluded ids in ascending order."""
    excl = sorted(set(int(e) for e in excl))
    P = n_items - len(excl)
    rows = np.arange(n_rows)
    picks = np.full((n_rows, F), -1, dtype=np.int64)
    for k in range(F):
        j = P - F + k
        hi = draw_key(seed, stream, rows, k) >> np.uint64(32)                       # < 2^32, so hi * (j + 1) < 2^63
        cand = ((hi * np.uint64(j + 1)) >> np.uint64(32)).astype(np.int64)
        taken = (picks[:, :k] == cand[:, None]).any(axis=1)
        picks[:, k] = np.where(taken, j, cand)
    out = picks.copy()
    for e in excl:
        out += (e <= out).astype(np.int64)
    return out
