"""Numpy restatement of the CatchSyncSelectUsers definition (include/recad_hip.h): integers as Python ints or int64, the fp64
steps in the written order, one rounding to fp32.  The kernels of csrc/catchsync.hip are compared with it word for word."""
import numpy as np

MAX_CELLS = 8192
BAD_FEATURE, TOO_MANY_CELLS = 17, 18
MODES = ("sync", "normality", "residual")


def bucket(x, s):
    """e * 2^s + m: e the index of x's leading one bit, m the s bits directly below it, zero-filled when e < s."""
    x = int(x)
    assert x >= 1 and 0 <= s <= 3
    e = 0
    while x >> (e + 1):
        e += 1
    m = (x >> (e - s) if e >= s else x << (s - e)) & ((1 << s) - 1)
    return e * (1 << s) + m


def features(ptr, idx, n_items):
    """(deg_item, reach) int64 [I]: the column lengths, and per column the sum of its users' row lengths."""
    ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    d = np.diff(ptr)
    rows = np.repeat(np.arange(len(d)), d)
    deg = np.bincount(idx, minlength=n_items).astype(np.int64)
    reach = np.zeros(n_items, dtype=np.int64)
    np.add.at(reach, idx, d[rows])
    return deg, reach


def key_of(deg, reach, s):
    return bucket(deg, s) * 65536 + bucket(reach, s)


def cells(deg, reach, s, cap=MAX_CELLS):
    """(cell_of int32 [I], cell_count int32 [cap], (M, N, SB, all_equal)), or ("refused", rule, item) of the lowest
    offending item.  Items that break BAD_FEATURE take no part in the ranking."""
    deg, reach = [int(x) for x in deg], [int(x) for x in reach]
    bad = [i for i in range(len(deg)) if deg[i] < 0 or reach[i] < 0 or (deg[i] > 0 and reach[i] == 0)]
    skip = set(bad)
    keys = {i: key_of(deg[i], reach[i], s) for i in range(len(deg)) if deg[i] >= 1 and i not in skip}
    rank = {k: c for c, k in enumerate(sorted(set(keys.values())))}
    over = [i for i, k in keys.items() if rank[k] >= cap]
    worst = min([(i, BAD_FEATURE) for i in bad] + [(i, TOO_MANY_CELLS) for i in over], default=None)
    if worst is not None:
        return "refused", worst[1], worst[0]
    cell_of = np.full(len(deg), -1, dtype=np.int32)
    count = np.zeros(cap, dtype=np.int32)
    for i, k in keys.items():
        cell_of[i] = rank[k]
        count[rank[k]] += 1
    M = len(rank)
    n_c = [int(c) for c in count[:M]]
    return cell_of, count, (M, sum(n_c), sum(c * c for c in n_c), int(len(set(n_c)) <= 1))


def user_sums(ptr, idx, cell_of, cell_count, M):
    """(pair_num, back_num) int64 [U]; an entry whose cell is -1 or >= M is skipped."""
    U = len(ptr) - 1
    pair, back = np.zeros(U, dtype=np.int64), np.zeros(U, dtype=np.int64)
    for u in range(U):
        c = np.asarray(cell_of, dtype=np.int64)[np.asarray(idx[ptr[u]:ptr[u + 1]], dtype=np.int64)]
        c = c[(c >= 0) & (c < M)]
        n_uc = np.bincount(c, minlength=1).astype(np.int64)
        pair[u] = int((n_uc * n_uc).sum())
        back[u] = int(np.asarray(cell_count, dtype=np.int64)[c].sum())
    return pair, back


def score_f64(d, pair, back, info, mode):
    """An eligible user's score before the rounding to fp32: Python floats are fp64 and every operation below rounds on its own."""
    M, N, SB, all_equal = (int(x) for x in info)
    fd, p, b, fM, fN, fSB = float(int(d)), float(int(pair)), float(int(back)), float(M), float(N), float(SB)
    if mode == "sync":
        return (p - fd) / (fd * (fd - 1.0))
    if mode == "normality":
        return b / (fd * fN)
    if mode != "residual":
        raise ValueError(mode)
    sy, n = p / (fd * fd), b / (fd * fN)
    if all_equal:
        s_min = 1.0 / fM
    else:
        s_b = fSB / (fN * fN)
        s_min = (((fM * n) * n - 2.0 * n) + s_b) / (fM * s_b - 1.0)
    return sy - s_min


def score_one(d, pair, back, info, mode, min_items):
    """One user's score as float32; exactly -1 below min_items."""
    return np.float32(-1.0) if int(d) < min_items else np.float32(score_f64(d, pair, back, info, mode))


def scores(ptr, pair, back, info, mode, min_items):
    d = np.diff(np.asarray(ptr, dtype=np.int64))
    return np.array([score_one(d[u], pair[u], back[u], info, mode, min_items) for u in range(len(d))], dtype=np.float32)


def run(ptr, idx, n_items, mode="sync", grid_bits=1, min_items=20):
    """The whole definition: dict of scores, pair_num, back_num, cell_of, cell_count, info, deg_item, reach."""
    deg, reach = features(ptr, idx, n_items)
    cell_of, count, info = cells(deg, reach, grid_bits)
    pair, back = user_sums(ptr, idx, cell_of, count, max(info[0], 1))
    return {"scores": scores(ptr, pair, back, info, mode, min_items), "pair_num": pair, "back_num": back, "cell_of": cell_of,
            "cell_count": count, "info": info, "deg_item": deg, "reach": reach}


def select(scores_, m):
    """The ids of the m largest scores, ties to the lower id."""
    s = np.asarray(scores_, dtype=np.float32) + np.float32(0)
    if not np.all(np.isfinite(s)) or not 0 <= m <= len(s):
        raise ValueError("a non-finite score, or m outside 0..n")
    return np.lexsort((np.arange(len(s)), -s))[:m].tolist()
