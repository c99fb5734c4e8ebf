"""Float64 numpy restatement of rk_rank_metrics (include/recad_hip.h): held-out Recall / Precision / NDCG / HitRate / MRR @k and
the per-user arrays behind them, vectorised, with the entry point's arguments -- plus the crafted rows both suites run.

Conventions (the LightGCN evaluation code's): recall over |gt|, precision over k, IDCG over min(k, |gt|) positions, a -1 pad
matches nothing, a user with an empty held-out list is not counted.  `idcg_over` / `recall_over` select the two WRONG forms the
host suite must be able to tell from the right one."""
import numpy as np


def discount_table(K):
    return 1.0 / np.log2(np.arange(K, dtype=np.float64) + 2.0)


def rank_metrics(top_ids, user_ids, gt_ptr, gt_idx, ks, discount, idcg_over="min", recall_over="gt"):
    """-> hits int32 [n, nk], dcg float64 [n, nk], first int32 [n], out float64 [1 + 5 nk] (sums, out[0] = counted rows)."""
    top_ids = np.asarray(top_ids, dtype=np.int64)
    n, K = top_ids.shape
    users = np.asarray(user_ids, dtype=np.int64)
    gt_ptr, gt_idx = np.asarray(gt_ptr, dtype=np.int64), np.asarray(gt_idx, dtype=np.int64)[: int(np.asarray(gt_ptr)[-1])]
    ks = np.clip(np.asarray(ks, dtype=np.int64), 1, K)
    discount = np.asarray(discount, dtype=np.float64)
    width = int(max(top_ids.max(initial=0), gt_idx.max(initial=0))) + 1
    rows = np.repeat(np.arange(len(gt_ptr) - 1, dtype=np.int64), np.diff(gt_ptr))
    member = np.isin(users[:, None] * width + top_ids, rows * width + gt_idx) & (top_ids >= 0)
    glen = np.diff(gt_ptr)[users] if n else np.zeros(0, dtype=np.int64)
    counted = glen > 0
    chits = np.cumsum(member, axis=1)
    cdcg = np.cumsum(member * discount[None, :], axis=1)
    hits = chits[:, ks - 1].astype(np.int32)
    dcg = cdcg[:, ks - 1]
    first = np.where(member.any(axis=1), member.argmax(axis=1), -1).astype(np.int32)
    cum = np.concatenate([[0.0], np.cumsum(discount)])
    out = np.zeros(1 + 5 * len(ks))
    out[0] = counted.sum()
    g = glen[counted].astype(np.float64)
    for q, k in enumerate(ks):
        h = hits[counted, q].astype(np.float64)
        ideal = cum[np.minimum(k, glen[counted])] if idcg_over == "min" else cum[k]
        f = first[counted]
        out[1 + 5 * q + 0] = np.sum(h / (g if recall_over == "gt" else np.minimum(k, g)))
        out[1 + 5 * q + 1] = np.sum(h / float(k))
        out[1 + 5 * q + 2] = np.sum(dcg[counted, q] / ideal)
        out[1 + 5 * q + 3] = np.sum(h > 0)
        out[1 + 5 * q + 4] = np.sum(np.where((f >= 0) & (f < k), 1.0 / np.maximum(f + 1.0, 1.0), 0.0))
    return hits, dcg, first, out


def cutoff_sets(K):
    """The four cut-off sets of the suites: {1}; {K}; {1, 64, 65, K} clipped to K and deduplicated; eight in descending order."""
    return [[1], [K], sorted(set(min(k, K) for k in (1, 64, 65, K))), [max(1, K - (i * K) // 8) for i in range(8)]]


N_USERS, N_ITEMS = 48, 640   # (items: more than twice the longest list, so a held-out list can be longer than K and still miss)


def crafted(K, n, seed=0):
    """(top_ids int32 [n, K], user_ids int32 [n], gt_ptr int32 [N_USERS + 1], gt_idx int32): 15 crafted rows, then random ones.
    n below 15 draws its rows from the crafted ones (seeded), so the small sizes still meet them.

    user 0 empty held-out list | 1 one held-out item, listed first | 2 held-out list longer than K | 3 the hit at 0 | 4 at 63 |
    5 at 64 | 6 at K - 1 (positions clipped to K - 1) | 7 every position a hit | 8 no hit | 9 a list of -1 only | 10 a -1 tail
    | 11 held-out items that are never listed (a seen item stays in |gt|) | 12 the highest item id, hit | 13 user 3 again with
    another list | 14 user 2 again."""
    rng = np.random.default_rng(1000 * K + n + seed)
    I = N_ITEMS
    gt = [np.zeros(0, dtype=np.int64) for _ in range(N_USERS)]
    lists = []

    def fresh(count, avoid):
        pool = np.setdiff1d(np.arange(I - 1), np.asarray(avoid, dtype=np.int64))   # (I - 1 is kept for user 12)
        return rng.choice(pool, size=count, replace=False)

    def one_hit(user, pos):
        pos = min(pos, K - 1)
        lst = fresh(K, gt[user])
        lst[pos] = gt[user][rng.integers(len(gt[user]))]
        return user, lst

    lists.append((0, fresh(K, [])))
    gt[1] = fresh(1, [])
    lists.append(one_hit(1, 0))
    gt[2] = np.sort(fresh(K + 7, []))
    lst = fresh(K, [])
    lists.append((2, lst))
    for u in (3, 4, 5, 6):
        gt[u] = np.sort(fresh(int(rng.integers(2, 9)), []))
    for u, pos in ((3, 0), (4, 63), (5, 64), (6, K - 1)):
        lists.append(one_hit(u, pos))
    lst = fresh(K, [])
    gt[7] = np.sort(lst)
    lists.append((7, lst))
    gt[8] = np.sort(fresh(5, []))
    lists.append((8, fresh(K, gt[8])))
    gt[9] = np.sort(fresh(4, []))
    lists.append((9, np.full(K, -1)))
    gt[10] = np.sort(fresh(6, []))
    lst = fresh(K, gt[10])
    lst[0] = gt[10][0]
    lst[(K + 1) // 2:] = -1
    lists.append((10, lst))
    gt[11] = np.sort(fresh(5, []))
    lst = fresh(K, gt[11])
    if K >= 2:
        lst[1] = gt[11][3]
    lst[K // 2] = gt[11][0]
    lists.append((11, lst))
    gt[12] = np.sort(np.append(fresh(2, []), I - 1))
    lst = fresh(K, gt[12])
    lst[K // 3] = I - 1
    lists.append((12, lst))
    lists.append(one_hit(3, K // 2))
    lists.append((2, np.roll(lists[2][1], 1)))
    for u in range(13, N_USERS):
        gt[u] = np.sort(rng.choice(I, size=int(rng.integers(0, 40)), replace=False))
    n_crafted = len(lists)
    while len(lists) < n:
        u = int(rng.integers(13, N_USERS))
        lst = rng.permutation(I)[:K]
        if len(gt[u]) and rng.random() < 0.5:     # (a random list rarely hits: plant a few)
            m = min(K, len(gt[u]), int(rng.integers(1, 6)))
            lst[rng.choice(K, size=m, replace=False)] = rng.choice(gt[u], size=m, replace=False)
            _, keep = np.unique(lst, return_index=True)
            dup = np.setdiff1d(np.arange(K), keep)
            lst[dup] = -1
        lists.append((u, lst))
    if n < n_crafted:
        lists = [lists[i] for i in rng.choice(n_crafted, size=n, replace=False)]
    gt_ptr = np.zeros(N_USERS + 1, dtype=np.int32)
    gt_ptr[1:] = np.cumsum([len(g) for g in gt])
    gt_idx = np.concatenate(gt).astype(np.int32)
    top_ids = np.stack([l for _, l in lists]).astype(np.int32).reshape(n, K)
    user_ids = np.asarray([u for u, _ in lists], dtype=np.int32)
    return top_ids, user_ids, gt_ptr, gt_idx
