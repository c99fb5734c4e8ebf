"""Restatement of the FraudarSelectUsers definition (include/recad_hip.h) on Python integers: the weight table, the peel twice
over (a lazy-deletion heap, and an O(N^2) scan that shares no code with it), the textbook float64 greedy on 1 / ln(d + 5), the
rounds of n_blocks, and the variants the definition rules out.  Nodes: user u is u, item i is U + i."""
import heapq
import math

import numpy as np

ONE = 1 << 24
MAX_NODES = 1 << 19
BAD_WEIGHT, BAD_DEGREE = 19, 20


def weight_table(U, kind, log_offset=5.0):
    """wtab uint32 [U + 1]: rint(2^24 / ln(d + log_offset)) in float64, or 2^24 throughout."""
    if kind == "degree":
        return np.full(U + 1, ONE, dtype=np.uint32)
    assert kind == "log"
    return np.array([min(float(np.rint(ONE / np.log(np.float64(d) + np.float64(log_offset)))), 2.0 ** 32 - 1) for d in range(U + 1)]).astype(np.uint32)


def degrees(idx, I):
    return np.bincount(np.asarray(idx, dtype=np.int64), minlength=I).astype(np.int64)


def weights(deg, kind, log_offset=5.0, U=None):
    """w_i = wtab[deg_i], uint32 [I]."""
    deg = np.asarray(deg, dtype=np.int64)
    tab = weight_table(int(deg.max(initial=0)) if U is None else U, kind, log_offset)
    return tab[deg]


def init(U, I, ptr, idx, wtab):
    """What rk_fd_init writes: (w_item uint32 [I], pri uint64 [U + I], f_0), or ("refused", rule, index)."""
    deg = degrees(idx, I)
    w = np.asarray(wtab, dtype=np.int64)[deg]
    bad = sorted(set(int(d) for d, x in zip(deg, w) if not 1 <= x <= ONE))
    if bad:
        return ("refused", BAD_WEIGHT, bad[0])
    pri = np.zeros(U + I, dtype=np.uint64)
    for u in range(U):
        pri[u] = int(w[np.asarray(idx[ptr[u]:ptr[u + 1]], dtype=np.int64)].sum())
    pri[U:] = (w * deg).astype(np.uint64)
    return w.astype(np.uint32), pri, int((w * deg).sum())


def _adjacency(U, I, ptr, idx):
    rows = [[int(i) for i in idx[ptr[u]:ptr[u + 1]]] for u in range(U)]
    cols = [[] for _ in range(I)]
    for u, r in enumerate(rows):
        for i in r:
            cols[i].append(u)
    return rows, cols


def _best(f_trace, N, latest=False):
    """t* = the least t maximising f_t / (N - t), by exact cross-multiplication (the latest one with `latest`)."""
    bt = 0
    for t in range(1, N):
        a, b = f_trace[t] * (N - bt), f_trace[bt] * (N - t)
        if a > b or (latest and a == b):
            bt = t
    return bt, f_trace[bt], N - bt


def peel(U, I, ptr, idx, w, tie_high=False, item_first=False, latest=False, charge_removed=False):
    """The peel with a lazy-deletion heap -> order, step_of, f_trace, (t*, f*, n*).  The keyword variants are the ones the
    definition rules out (tests only): ties to the higher id; an item before a user on a tie; the latest maximum; a removed
    neighbour still charged (f loses every edge of v, those whose other end has gone included)."""
    N = U + I
    w = [int(x) for x in w]
    rows, cols = _adjacency(U, I, ptr, idx)
    pri = [sum(w[i] for i in rows[u]) for u in range(U)] + [w[i] * len(cols[i]) for i in range(I)]
    full = list(pri)
    f = sum(pri[:U])

    def key(v):
        k = v
        if item_first:
            k = v - U if v >= U else v + I
        return (pri[v], -k if tie_high else k, v)

    heap = [key(v) for v in range(N)]
    heapq.heapify(heap)
    alive = [True] * N
    order, step_of, f_trace = [], [0] * N, []
    for t in range(N):
        while True:
            p, _, v = heapq.heappop(heap)
            if alive[v] and p == pri[v]:
                break
        order.append(v)
        step_of[v] = t
        f_trace.append(f)
        f -= full[v] if charge_removed else pri[v]
        alive[v] = False
        if v < U:
            for i in rows[v]:
                if alive[U + i]:
                    pri[U + i] -= w[i]
                    heapq.heappush(heap, key(U + i))
        else:
            for u in cols[v - U]:
                if alive[u]:
                    pri[u] -= w[v - U]
                    heapq.heappush(heap, key(u))
    if charge_removed:
        f_trace = [max(x, 0) for x in f_trace]
    return (np.array(order, dtype=np.int32), np.array(step_of, dtype=np.int32), np.array(f_trace, dtype=np.uint64), _best(f_trace, N, latest))


def peel_scan(U, I, ptr, idx, w, alive_tab=None):
    """The same by the definition's letter: every step scans all alive nodes and recounts every priority from the edges.
    alive_tab (a variant the definition rules out): the weights of every step are alive_tab[the item's ALIVE degree]."""
    N = U + I
    edges = [(u, int(idx[e])) for u in range(U) for e in range(int(ptr[u]), int(ptr[u + 1]))]
    gone = set()
    order, step_of, trace = [], {}, []
    for t in range(N):
        pr = {v: 0 for v in range(N) if v not in gone}
        if alive_tab is not None:
            deg = [0] * I
            for u, i in edges:
                if u not in gone and (U + i) not in gone:
                    deg[i] += 1
            w = [int(alive_tab[d]) for d in deg]
        for u, i in edges:
            if u not in gone and (U + i) not in gone:
                pr[u] += int(w[i])
                pr[U + i] += int(w[i])
        trace.append(sum(p for v, p in pr.items() if v < U))
        v = min(pr, key=lambda x: (pr[x], x))
        order.append(v)
        step_of[v] = t
        gone.add(v)
    bt = max(range(N), key=lambda t: (FractionLike(trace[t], N - t), -t))
    return (np.array(order, dtype=np.int32), np.array([step_of[v] for v in range(N)], dtype=np.int32), np.array(trace, dtype=np.uint64),
            (bt, trace[bt], N - bt))


class FractionLike:
    """f / n ordered exactly, for peel_scan's argmax."""

    def __init__(self, f, n):
        self.f, self.n = f, n

    def __lt__(self, o):
        return self.f * o.n < o.f * self.n

    def __eq__(self, o):
        return self.f * o.n == o.f * self.n

    def __gt__(self, o):
        return self.f * o.n > o.f * self.n


def textbook(U, I, ptr, idx, log_offset=5.0):
    """The float64 greedy of the paper on w_i = 1 / ln(deg_i + 5): (users, items) of the best block, ties to the lower id."""
    N = U + I
    rows, cols = _adjacency(U, I, ptr, idx)
    w = np.array([1.0 / math.log(len(c) + log_offset) for c in cols])
    pri = np.array([sum(w[i] for i in rows[u]) for u in range(U)] + [w[i] * len(cols[i]) for i in range(I)], dtype=np.float64)
    f = float(sum(w[i] * len(cols[i]) for i in range(I)))
    alive = np.ones(N, dtype=bool)
    best, best_t, step_of = -1.0, 0, np.zeros(N, dtype=np.int64)
    for t in range(N):
        if f / (N - t) > best:
            best, best_t = f / (N - t), t
        v = int(np.argmin(np.where(alive, pri, np.inf)))
        step_of[v] = t
        alive[v] = False
        f -= pri[v]
        if v < U:
            for i in rows[v]:
                if alive[U + i]:
                    pri[U + i] -= w[i]
        else:
            for u in cols[v - U]:
                if alive[u]:
                    pri[u] -= w[v - U]
    members = np.nonzero(step_of >= best_t)[0]
    return members[members < U], members[members >= U] - U


def block_of(step_of, t_best, U):
    members = np.nonzero(np.asarray(step_of) >= t_best)[0].astype(np.int64)
    return members[members < U], members[members >= U] - U


def select_count(order, U, m):
    """The m users removed last, last first."""
    o = np.asarray(order)[::-1]
    return o[o < U][:m].astype(np.int64).tolist()


def drop_block(U, ptr, idx, users, items):
    """The CSR without the edges that have both ends in the block."""
    in_u, in_i = set(int(u) for u in users), set(int(i) for i in items)
    rows = [[int(i) for i in idx[ptr[u]:ptr[u + 1]] if not (u in in_u and int(i) in in_i)] for u in range(U)]
    new_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return new_ptr, np.array([i for r in rows for i in r], dtype=np.int64)


def blocks(U, I, ptr, idx, kind="log", log_offset=5.0, n_blocks=1):
    """The rounds of n_blocks: [{users, items, t_best, f_best, n_best, density}], weights recomputed from each round's degrees."""
    out = []
    ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    for _ in range(n_blocks):
        if len(idx) == 0:
            break
        w = weight_table(U, kind, log_offset)[degrees(idx, I)]
        _, step_of, _, (t, f, n) = peel(U, I, ptr, idx, w)
        if f == 0:
            break
        users, items = block_of(step_of, t, U)
        out.append({"users": users, "items": items, "t_best": t, "f_best": f, "n_best": n, "density": f / (n * float(ONE))})
        ptr, idx = drop_block(U, ptr, idx, users, items)
    return out


def flagged(U, I, ptr, idx, kind="log", log_offset=5.0, select="block", n_blocks=1, m=0):
    """What defense_step returns."""
    if len(idx) == 0:
        return []
    if select == "count":
        w = weight_table(U, kind, log_offset)[degrees(idx, I)]
        order, _, _, (_, f, _) = peel(U, I, ptr, idx, w)
        return select_count(order, U, m) if f else []
    out = []
    for b in blocks(U, I, ptr, idx, kind, log_offset, n_blocks):
        out += [u for u in b["users"].tolist() if u not in set(out)]
    return out


def g_of(U, I, ptr, idx, w, members):
    """g(S) = (the weight of the edges inside S) / |S| as (numerator, denominator)."""
    s = set(int(v) for v in members)
    f = sum(int(w[int(i)]) for u in range(U) if u in s for i in idx[ptr[u]:ptr[u + 1]] if U + int(i) in s)
    return f, len(s)
