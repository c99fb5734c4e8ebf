"""Seeded differential sweep of the kernels that consume "the U x I rating CSR under the rules of rk_knn_norms": the DegSim,
ItemKNN, UserKNN, RP3beta and CatchSync entries of include/recad_hip.h against their numpy restatements (tests/_knn_restate.py,
_itemknn_restate.py, _userknn_restate.py, _rp3_restate.py, _catchsync_restate.py), every drawn parameter at once.

case(seed, index) builds one rating CSR and every drawn parameter from np.random.default_rng([seed, index]) alone, so a failure
report's (seed, index) rebuilds the case anywhere.  The generator stays inside every entry's contract: nothing here provokes a
refusal or an unchecked read.  expected(c, leg) is the host side of a leg (restatements only, no device); run(seed, n_cases, leg)
is one device pass per case and raises on the first difference with the seed, the index, the drawn parameters and the first
differing indices.  Everything is compared exactly: integers as integers, floats by bit pattern.  The one place where the
definition itself is not exact is the double pow of rk_rp3_steps / rk_rp3_factors at an exponent other than 0 and 1: there P may
differ from numpy's by one unit and a factor by POW_ULP units (the allowances of tests/test_rp3beta_kernels_gpu.py), and the
tables are restated from the P, fa and fb the device wrote, to the bit.

Host time of a leg alone (case() plus expected() on a CPU, no device), measured with the counts of N_CASES, each under 5 s:
    neighbours  200 cases  3.7 s
    rp3         120 cases  3.3 s
    catchsync   400 cases  1.1 s

    python tests/tools/csr_kernel_sweep.py SEED N_CASES LEG      # on the GPU box"""
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, ".")
from tests import _catchsync_restate as CR
from tests import _itemknn_restate as IR
from tests import _knn_restate as K
from tests import _rp3_restate as PR
from tests import _userknn_restate as UR

LEGS = ("neighbours", "rp3", "catchsync")
SEED = 20261021
N_CASES = {"neighbours": 200, "rp3": 120, "catchsync": 400}            # the host side of each leg stays under 5 s (docstring)
KS = (1, 2, 7, 25, 64, 127, 128)
BANDS = (0, 64, 128, 192, 320)
ORDERS = ("null", "identity", "reversed", "random")
USER_BLOCKS = (0, 1, 2, 3, 8, 16)
EXPONENTS = (0.0, 1.0, 0.5, 0.8, 1.7, 4.0)                           # 4: the only drawn alpha at which a step rounds to 0
FORMS = ("auto", "wave", "workgroup")
MIN_ITEMS = (2, 5, 20)
KINDS = ("sparse", "dense-wide", "tiny", "blocks")
N_PAIRS = 200
POW_ULP = 17.0


# ------------------------------------------------------------------------------------------------------------------ generator
def _copies(rng, A, axis):
    """1 to 3 groups of identical columns (axis 1) or rows (axis 0), 2..40 wide, half of them across a multiple of 64."""
    n = A.shape[axis]
    for _ in range(int(rng.integers(1, 4))):
        w = int(min(rng.integers(2, 41), n))
        a = int(rng.integers(0, n - w + 1))
        edges = np.arange(64, n, 64)
        if len(edges) and w >= 2 and rng.random() < 0.5:
            a = int(np.clip(int(rng.choice(edges)) - int(rng.integers(1, w)), 0, n - w))
        if axis == 1:
            A[:, a:a + w] = A[:, [a]]
        else:
            A[a:a + w] = A[[a]]


def _matrix(rng):
    kind = KINDS[int(rng.choice(4, p=[0.3, 0.3, 0.15, 0.25]))]
    if kind == "sparse":
        U, I, density = int(rng.integers(1, 301)), int(rng.integers(1, 301)), rng.uniform(0.01, 0.3)
    elif kind == "dense-wide":
        U, I, density = int(rng.integers(8, 41)), int(rng.integers(300, 701)), rng.uniform(0.3, 0.7)
    elif kind == "tiny":
        U, I, density = int(rng.integers(1, 9)), int(rng.integers(1, 131)), rng.uniform(0.05, 0.9)
    else:
        U, I, density = int(rng.integers(4, 161)), int(rng.integers(4, 401)), rng.uniform(0.05, 0.4)
    implicit = bool(rng.random() < 0.4)
    A = (rng.random((U, I)) < density).astype(np.int64)
    if not implicit:
        A *= rng.integers(1, 6, size=(U, I))
    if rng.random() < 0.2 and A.any():
        r, c = np.nonzero(A)
        hit = rng.integers(0, len(r), size=int(rng.integers(1, 13)))
        A[r[hit], c[hit]] = 127
        u = int(r[hit[0]])                                             # and a heavy row: all but a few of that row's entries
        A[u] = np.where((A[u] > 0) & (rng.random(I) < 0.8), 127, A[u])
    if kind == "blocks":
        _copies(rng, A, 1)
        _copies(rng, A, 0)
    empty_row = int(rng.integers(0, U)) if rng.random() < 0.5 else -1
    empty_col = int(rng.integers(0, I)) if rng.random() < 0.5 else -1
    if empty_row >= 0:
        A[empty_row] = 0
    if empty_col >= 0:
        A[:, empty_col] = 0
    return kind, implicit, A


def order_of(kind, perm):
    """The `order` argument of a drawn kind over len(perm) rows: None, or a true permutation."""
    n = len(perm)
    return {"null": None, "identity": np.arange(n), "reversed": np.arange(n)[::-1], "random": perm}[kind]


def case(seed, index):
    """One case: the CSR (ptr int32, idx int32, val float32), U, I and every drawn parameter, from rng([seed, index]) alone."""
    rng = np.random.default_rng([seed, index])
    kind, implicit, A = _matrix(rng)
    U, I = A.shape
    rows = [np.nonzero(a)[0] for a in A]
    c = {"seed": seed, "index": index, "kind": kind, "implicit": implicit, "U": U, "I": I,
         "ptr": np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32),
         "idx": np.concatenate(rows + [np.zeros(0, dtype=np.int64)]).astype(np.int32),
         "val": np.concatenate([a[r] for a, r in zip(A, rows)] + [np.zeros(0, dtype=np.int64)]).astype(np.float32)}
    pick = lambda options: options[int(rng.integers(0, len(options)))]
    c["k"] = pick(KS)
    for name in ("band_fit", "band_fit2", "band_score", "band_score2"):
        c[name] = pick(BANDS)
    for name in ("order", "order2"):
        c[name] = pick(ORDERS)
        c[name + "_users"], c[name + "_items"] = rng.permutation(U), rng.permutation(I)
    c["user_block"], c["user_block2"] = pick(USER_BLOCKS), pick(USER_BLOCKS)
    c["normalize"] = int(rng.integers(0, 2))
    c["alpha"], c["beta"] = pick(EXPONENTS), pick(EXPONENTS)
    c["grid_bits"], c["form"], c["mode"], c["min_items"] = int(rng.integers(0, 4)), int(rng.integers(0, 3)), int(rng.integers(0, 3)), pick(MIN_ITEMS)
    c["m_select"] = int(rng.integers(0, U + 1))
    # the users scored: in range, repeats, a user with an empty row when there is one; the other scoring entries also take ids
    # outside [0, U), for which the header defines the result
    ids = rng.integers(0, U, size=int(rng.integers(1, 13)))
    empty = np.nonzero(np.diff(c["ptr"]) == 0)[0]
    if len(empty):
        ids[int(rng.integers(0, len(ids)))] = empty[int(rng.integers(0, len(empty)))]
    ids = np.concatenate([ids, ids[: int(rng.integers(0, 3))]])
    c["user_ids"] = ids.astype(np.int32)
    c["score_ids"] = np.concatenate([ids, [-1, U, 2 ** 30]])[rng.permutation(len(ids) + 3)].astype(np.int32)
    pu, pi = ids[rng.integers(0, len(ids), size=N_PAIRS)].astype(np.int64), rng.integers(0, I, size=N_PAIRS)
    bad = [(-1, 0), (U, 0), (0, -1), (0, I), (2 ** 40, 0), (0, 2 ** 40), (-2 ** 40, -2 ** 40), (U, I)]
    for p, (u, i) in zip(rng.permutation(N_PAIRS)[: len(bad)], bad):
        pu[p], pi[p] = (u if u else pu[p]), (i if i else pi[p])
    c["pair_users"], c["pair_items"] = pu, pi
    # RP3beta: a hand-made P / fa / fb for a second neighbour call (the entry takes any table of positive P).  Sums of a few P
    # of 18..23 bits have 25 and more significant bits, and factors one or two units from 1 put the double product next to a
    # tie of the fp32 rounding: there the order of the three double multiplies shows in the rounded weight
    c["hand"] = None
    if rng.random() < 0.35:
        units = np.array([0, 1, 2, 3, -0.5, -1, -1.5]) * 2.0 ** -52
        c["hand"] = {"P": rng.integers(2 ** 18, 2 ** 23, size=len(c["idx"])).astype(np.int64),
                     "fa": 1.0 + units[rng.integers(0, len(units), size=I)], "fb": 1.0 + units[rng.integers(0, len(units), size=I)]}
    return c


def params(c):
    """The scalars of a case, for a failure report."""
    return {k: v for k, v in c.items() if not isinstance(v, (np.ndarray, dict))} | {"nnz": len(c["idx"]), "hand": c["hand"] is not None}


def transpose(ptr, idx, val, n_items):
    """The transposed CSR as rk_pca_transpose writes it: users ascending inside a column."""
    row = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    o = np.lexsort((row, idx))
    colptr = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n_items))]).astype(np.int32)
    return colptr, row[o].astype(np.int32), val[o].astype(np.float32)


def csr(c):
    return c["ptr"], c["idx"], c["val"], c["I"]


# ------------------------------------------------------------------------------------------------------------------ host side
def _in_range_scores(fn, c, ids, *args):
    """A restated score matrix for ids of which some lie outside [0, U): those rows are +0.0."""
    ids = np.asarray(ids, dtype=np.int64)
    ok = (ids >= 0) & (ids < c["U"])
    out = np.zeros((len(ids), c["I"]), dtype=np.float32)
    if ok.any():
        out[ok] = fn(*csr(c), *args, ids[ok])
    return out


def expect_neighbours(c):
    k, e = c["k"], {}
    A = K.dense(*csr(c))
    e["rnorm_user"], e["rnorm_item"] = K.rnorm(A), IR.item_rnorm(A)
    e["colptr"], e["crow"], e["cval"] = transpose(*csr(c))
    e["item_id"], e["item_w"] = IR.neighbours(*csr(c), k)
    e["user_id"], e["user_w"] = UR.neighbours(*csr(c), k)
    e["item_scores"] = IR.scores(*csr(c), e["item_id"], e["item_w"], c["user_ids"])
    e["item_pairs"] = IR.pair_scores(*csr(c), e["item_id"], e["item_w"], c["pair_users"], c["pair_items"])
    e["user_scores"] = UR.scores(*csr(c), e["user_id"], e["user_w"], c["score_ids"], c["normalize"])
    e["user_pairs"] = UR.pair_scores(*csr(c), e["user_id"], e["user_w"], c["pair_users"], c["pair_items"], c["normalize"])
    e["topw"], e["degsim"] = K.degsim(*csr(c), k)
    return e


def rp3_tables(c, P, fa, fb):
    S = PR.dots(c["ptr"], c["idx"], P, c["I"])
    return PR.neighbours_from(S, PR.weights(S, fa, fb), c["k"])


def expect_rp3(c, parts=None):
    """parts: the (P, fa, fb) the device wrote; None: the definition's own (numpy's pow)."""
    e = {}
    e["P"], e["r"] = PR.steps(c["ptr"], c["idx"], c["val"], c["alpha"])
    e["fa"], e["fb"] = PR.factors(np.bincount(c["idx"], minlength=c["I"]), c["alpha"], c["beta"])
    P, fa, fb = (e["P"], e["fa"], e["fb"]) if parts is None else parts
    e["nbr_id"], e["nbr_w"] = rp3_tables(c, P, fa, fb)
    if c["hand"] is not None:
        e["hand_id"], e["hand_w"] = rp3_tables(c, c["hand"]["P"], c["hand"]["fa"], c["hand"]["fb"])
    e["scores"] = _in_range_scores(PR.scores, c, c["score_ids"], e["nbr_id"], e["nbr_w"])
    e["pairs"] = PR.pair_scores(*csr(c), e["nbr_id"], e["nbr_w"], c["pair_users"], c["pair_items"])
    return e


def expect_catchsync(c):
    e = {}
    e["deg_item"], e["reach"] = CR.features(c["ptr"], c["idx"], c["I"])
    e["cell_of"], e["cell_count"], info = CR.cells(e["deg_item"], e["reach"], c["grid_bits"])
    e["info"] = np.array(info, dtype=np.int64)
    e["pair_num"], e["back_num"] = CR.user_sums(c["ptr"], c["idx"], e["cell_of"], e["cell_count"], max(info[0], 1))
    e["scores"] = CR.scores(c["ptr"], e["pair_num"], e["back_num"], info, CR.MODES[c["mode"]], c["min_items"])
    e["selected"] = np.array(CR.select(e["scores"], c["m_select"]), dtype=np.int32)
    return e


EXPECT = {"neighbours": expect_neighbours, "rp3": expect_rp3, "catchsync": expect_catchsync}


def expected(c, leg):
    return EXPECT[leg](c)


# ------------------------------------------------------------------------------------------------------------------ reach
def _list_reach(cand, W, k, bands):
    """Of one side's lists (cand bool [n, n] without the diagonal, W its weights): a tie exactly at the cut, a band of more than
    256 candidates under one of `bands`, a padded list, more than one band."""
    n = cand.shape[0]
    k_eff = min(k, n - 1)
    tie = False
    for i in np.nonzero(cand.sum(axis=1) > k_eff)[0] if k_eff else ():
        w = -np.sort(-W[i, cand[i]])
        if w[k_eff - 1] == w[k_eff]:
            tie = True
            break
    over = any(max(int(cand[:, a:a + (b or n)].sum(axis=1).max()) for a in range(0, n, b or n)) > 256 for b in bands)
    return {"tie_at_cut": tie, "over_256": over, "padded": bool((cand.sum(axis=1) < k).any()), "bands": any(0 < b < n for b in bands)}


def reach(c, leg):
    """Which of the paths the issue names this case takes, judged by the restatements alone."""
    A = K.dense(*csr(c))
    bands = (c["band_fit"], c["band_fit2"])
    if leg == "catchsync":
        e = expect_catchsync(c)
        M = int(e["info"][0])
        return {"form_" + FORMS[c["form"]]: True, "mode_" + CR.MODES[c["mode"]]: True, "cells_unequal": M > 1 and not e["info"][3],
                "cells_all_equal": M >= 1 and bool(e["info"][3])}
    if leg == "rp3":
        P, _, fa, fb = PR.fit_parts(c["ptr"], c["idx"], c["val"], c["I"], c["alpha"], c["beta"])
        S = PR.dots(c["ptr"], c["idx"], P, c["I"])
        cand = S > 0
        np.fill_diagonal(cand, False)
        return _list_reach(cand, PR.weights(S, fa, fb), c["k"], bands)
    out = {}
    for side, (D, W) in (("item", IR.similarities(A)), ("user", UR.similarities(A))):
        cand = D > 0
        np.fill_diagonal(cand, False)
        for name, hit in _list_reach(cand, W, c["k"], bands).items():
            out[name] = out.get(name, False) or hit
    # rk_userknn_scores: a kept neighbour's row is searched when it is longer than 128 and the band is narrower than the catalogue
    ids, d = UR.neighbours(*csr(c), c["k"])[0][:, c["user_ids"]], np.diff(c["ptr"])
    kept = d[ids[ids >= 0]]
    banded = any(0 < b < c["I"] for b in (c["band_score"], c["band_score2"]))
    out["row_searched"], out["row_strided"] = bool(banded and (kept > 128).any()), bool((kept <= 128).any())
    return out


# ------------------------------------------------------------------------------------------------------------------ device side
class Mismatch(AssertionError):
    pass


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def difference(got, want, sentinel=-777):
    """None when `got` is `want` exactly (integers as integers, floats by bit pattern, so -0.0 is not +0.0), else what differs
    and where first.  `want` holds no sentinel (NaN for floats), so equality also says that every element was written."""
    got, want = np.asarray(got), np.asarray(want)
    assert not (np.isnan(want).any() if want.dtype.kind == "f" else (want == sentinel).any()), "a sentinel in the expected output"
    if got.shape != want.shape or got.dtype.kind != want.dtype.kind or (got.dtype.kind == "f" and got.dtype != want.dtype):
        return f"shape / type {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    ne = _bits(got) != _bits(want.astype(got.dtype))
    if not ne.any():
        return None
    where = np.argwhere(ne)[:5]
    pick = tuple(where.T)
    return f"{int(ne.sum())} of {ne.size} elements differ, first at {where.tolist()}: got {got[pick].tolist()}, want {want[pick].tolist()}"


class _Device:
    """The calls of one case: guarded outputs (tests/test_knn_kernels_gpu.Out: sentinel prefill, 64-element margins), inputs held
    until the case ends, every comparison exact."""

    def __init__(self, c, dev):
        import torch
        from recad_amd import _lib
        from tests.test_knn_kernels_gpu import SENTINEL, Out, _dev
        self.c, self.dev, self.torch, self.L, self.P, self.Out, self.SENTINEL = c, dev, torch, _lib.lib(), _lib.ptr, Out, SENTINEL
        self.s = _lib.stream_ptr(dev)
        self.held = []
        self._up = _dev

    def up(self, a, dtype=None):
        if a is None:
            return None
        t = self._up(np.asarray(a, dtype=dtype), self.dev)
        self.held.append(t)
        return self.P(t)

    def out(self, n, dtype):
        o = self.Out(n, getattr(self.torch, dtype), self.dev)
        self.held.append(o)
        return o

    def fail(self, what, detail):
        raise Mismatch(f"{what}: {detail}\n  rebuild with case({self.c['seed']}, {self.c['index']}); drawn: {params(self.c)}")

    def call(self, name, *args):
        rc = getattr(self.L, name)(*args, self.s)
        if rc != 0:
            self.fail(name, f"returned {rc}: {self.L.rk_last_error().decode()}")

    def read(self, name, o, shape=None):
        """The written part of a guarded output; its margin must be as it was."""
        try:
            a = o.host()
        except AssertionError as err:
            self.fail(name, str(err))
        return a if shape is None else a.reshape(shape)

    def same(self, name, got, want):
        detail = difference(got, want, self.SENTINEL)
        if detail is not None:
            self.fail(name, detail)

    def pairs_in_matrix(self, name, pairs, matrix, row_ids):
        """Every pair with ids in range equals the matrix entry of its user's first row in the block."""
        c = self.c
        u, i = c["pair_users"], c["pair_items"]
        ok = (u >= 0) & (u < c["U"]) & (i >= 0) & (i < c["I"])
        first = {int(x): b for b, x in reversed(list(enumerate(row_ids)))}
        rows = np.array([first[int(x)] for x in u[ok]], dtype=np.int64)
        self.same(name + " against the matrix entries", pairs[ok], matrix[rows, i[ok]])
        if not (_bits(pairs[~ok]) == 0).all():
            self.fail(name, "a pair with an id out of range does not score +0.0")


def _csr_up(d):
    c = d.c
    return d.up(c["ptr"]), d.up(c["idx"]), d.up(c["val"])


def _order_up(d, kind, perm):
    o = order_of(kind, perm)
    return None if o is None else d.up(o, np.int32)


def run_neighbours(c, dev):
    d = _Device(c, dev)
    e = expect_neighbours(c)
    U, I, k, P = c["U"], c["I"], c["k"], d.P
    nnz = len(c["idx"])
    ptr, idx, val = _csr_up(d)
    # rk_knn_norms on the matrix, rk_pca_transpose, rk_knn_norms on the transpose the device wrote
    rn_u, rn_i, st = d.out(U, "float32"), d.out(I, "float32"), d.out(2, "int32")
    d.call("rk_knn_norms", U, I, ptr, idx, val, P(rn_u.full), P(st.full))
    d.same("rk_knn_norms status", d.read("status", st), [0, -1])
    d.same("rk_knn_norms rnorm", d.read("rnorm", rn_u), e["rnorm_user"])
    t = [d.out(I + 1, "int32"), d.out(nnz, "int32"), d.out(nnz, "float32")]
    d.call("rk_pca_transpose", U, I, ptr, idx, val, *(P(x.full) for x in t))
    for name, o in zip(("colptr", "crow", "cval"), t):
        d.same("rk_pca_transpose " + name, d.read(name, o), e[name])
    colptr, crow, cval = (P(x.full) for x in t)
    st2 = d.out(2, "int32")
    d.call("rk_knn_norms", I, U, colptr, crow, cval, P(rn_i.full), P(st2.full))
    d.same("rk_knn_norms (transpose) status", d.read("status", st2), [0, -1])
    d.same("rk_knn_norms (transpose) rnorm", d.read("rnorm", rn_i), e["rnorm_item"])

    def fit(side, band, order_kind, perm):
        n = I if side == "item" else U
        ids, w = d.out(k * n, "int32"), d.out(k * n, "float32")
        order = _order_up(d, order_kind, perm)
        if side == "item":
            d.call("rk_itemknn_neighbors", U, I, ptr, idx, val, colptr, crow, cval, P(rn_i.full), k, band, order, P(ids.full), P(w.full))
        else:                                                          # the UserKNN fit: the transposed roles
            d.call("rk_itemknn_neighbors", I, U, colptr, crow, cval, ptr, idx, val, P(rn_u.full), k, band, order, P(ids.full), P(w.full))
        return ids, w, d.read(side + " nbr_id", ids, (k, n)), d.read(side + " nbr_w", w, (k, n))

    tables = {}
    for side in ("item", "user"):
        ids, w, got_id, got_w = fit(side, c["band_fit"], c["order"], c["order_" + side + "s"])
        d.same(f"rk_itemknn_neighbors ({side} side) nbr_id", got_id, e[side + "_id"])
        d.same(f"rk_itemknn_neighbors ({side} side) nbr_w", got_w, e[side + "_w"])
        _, _, again_id, again_w = fit(side, c["band_fit2"], c["order2"], c["order2_" + side + "s"])
        d.same(f"rk_itemknn_neighbors ({side} side) nbr_id under band {c['band_fit2']} and order {c['order2']}", again_id, got_id)
        d.same(f"rk_itemknn_neighbors ({side} side) nbr_w under band {c['band_fit2']} and order {c['order2']}", again_w, got_w)
        tables[side] = (P(ids.full), P(w.full), got_w)
    pu, pi = d.up(c["pair_users"], np.int64), d.up(c["pair_items"], np.int64)
    # ItemKNN scoring from the device's own tables
    ids, nb = d.up(c["user_ids"], np.int32), len(c["user_ids"])
    mats = []
    for ub in (c["user_block"], c["user_block2"]):
        o = d.out(nb * I, "float32")
        d.call("rk_itemknn_scores", I, k, tables["item"][0], tables["item"][1], ptr, idx, val, nb, ids, ub, P(o.full))
        mats.append(d.read("rk_itemknn_scores", o, (nb, I)))
    d.same("rk_itemknn_scores", mats[0], e["item_scores"])
    d.same(f"rk_itemknn_scores under user_block {c['user_block2']}", mats[1], mats[0])
    o = d.out(N_PAIRS, "float32")
    d.call("rk_itemknn_pair_scores", I, U, k, tables["item"][0], tables["item"][1], ptr, idx, val, pu, pi, N_PAIRS, P(o.full))
    got = d.read("rk_itemknn_pair_scores", o)
    d.same("rk_itemknn_pair_scores", got, e["item_pairs"])
    d.pairs_in_matrix("rk_itemknn_pair_scores", got, mats[0], c["user_ids"])
    # UserKNN scoring
    ids, nb = d.up(c["score_ids"], np.int32), len(c["score_ids"])
    mats = []
    for band in (c["band_score"], c["band_score2"]):
        o = d.out(nb * I, "float32")
        d.call("rk_userknn_scores", U, I, k, tables["user"][0], tables["user"][1], ptr, idx, val, nb, ids, c["normalize"], band, P(o.full))
        mats.append(d.read("rk_userknn_scores", o, (nb, I)))
    d.same("rk_userknn_scores", mats[0], e["user_scores"])
    d.same(f"rk_userknn_scores under band {c['band_score2']}", mats[1], mats[0])
    o = d.out(N_PAIRS, "float32")
    d.call("rk_userknn_pair_scores", I, U, k, tables["user"][0], tables["user"][1], ptr, idx, val, pu, pi, N_PAIRS, c["normalize"], P(o.full))
    got = d.read("rk_userknn_pair_scores", o)
    d.same("rk_userknn_pair_scores", got, e["user_pairs"])
    d.pairs_in_matrix("rk_userknn_pair_scores", got, mats[0], c["score_ids"])
    # DegSim, and its topw against the UserKNN tables' kept weights
    topw, deg = d.out(U * k, "float32"), d.out(U, "float32")
    d.call("rk_knn_degsim", U, I, ptr, idx, val, colptr, crow, cval, P(rn_u.full), k, c["band_fit"],
           _order_up(d, c["order"], c["order_users"]), P(topw.full), P(deg.full))
    got_topw = d.read("topw", topw, (U, k))
    d.same("rk_knn_degsim topw", got_topw, e["topw"])
    d.same("rk_knn_degsim degsim", d.read("degsim", deg), e["degsim"])
    d.same("the UserKNN tables' kept weights against topw", tables["user"][2].T, got_topw)


def run_rp3(c, dev):
    d = _Device(c, dev)
    U, I, k, P = c["U"], c["I"], c["k"], d.P
    nnz = len(c["idx"])
    ptr, idx, val = _csr_up(d)
    colptr_h, crow_h, _ = transpose(*csr(c))
    colptr, crow = d.up(colptr_h), d.up(crow_h)
    Pd, r, fa, fb = d.out(nnz, "int64"), d.out(U, "int64"), d.out(I, "float64"), d.out(I, "float64")
    d.call("rk_rp3_steps", U, ptr, val, c["alpha"], P(Pd.full), P(r.full))
    d.call("rk_rp3_factors", I, colptr, c["alpha"], c["beta"], P(fa.full), P(fb.full))
    parts = (d.read("P", Pd).copy(), d.read("fa", fa).copy(), d.read("fb", fb).copy())
    e = expect_rp3(c, parts)
    d.same("rk_rp3_steps r", d.read("r", r), e["r"])
    if c["alpha"] in (0, 1):
        d.same("rk_rp3_steps P", parts[0], e["P"])
    elif nnz and (np.abs(parts[0] - e["P"]).max() > 1 or parts[0].min() < 1):
        d.fail("rk_rp3_steps P", f"beyond one unit of the definition's at {np.argwhere(np.abs(parts[0] - e['P']) > 1)[:5].tolist()}")
    for name, exponent, got in (("fa", c["alpha"], parts[1]), ("fb", c["beta"], parts[2])):
        if exponent in (0, 1):
            d.same("rk_rp3_factors " + name, got, e[name])
        else:
            ulps = np.abs(got - e[name]) / np.spacing(np.where(e[name] > 0, e[name], 1.0))
            if not (ulps <= POW_ULP).all() or (_bits(got)[e[name] == 0] != 0).any():
                d.fail("rk_rp3_factors " + name, f"beyond {POW_ULP} units of the definition's at {np.argwhere(~(ulps <= POW_ULP))[:5].tolist()}")

    def fit(table, fa_p, fb_p, band, order_kind, perm):
        ids, w = d.out(k * I, "int32"), d.out(k * I, "float32")
        d.call("rk_rp3_neighbors", U, I, ptr, idx, table, colptr, crow, fa_p, fb_p, k, band, _order_up(d, order_kind, perm),
               P(ids.full), P(w.full))
        return ids, w, d.read("nbr_id", ids, (k, I)), d.read("nbr_w", w, (k, I))

    ids, w, got_id, got_w = fit(P(Pd.full), P(fa.full), P(fb.full), c["band_fit"], c["order"], c["order_items"])
    d.same("rk_rp3_neighbors nbr_id", got_id, e["nbr_id"])
    d.same("rk_rp3_neighbors nbr_w", got_w, e["nbr_w"])
    _, _, again_id, again_w = fit(P(Pd.full), P(fa.full), P(fb.full), c["band_fit2"], c["order2"], c["order2_items"])
    d.same(f"rk_rp3_neighbors nbr_id under band {c['band_fit2']} and order {c['order2']}", again_id, got_id)
    d.same(f"rk_rp3_neighbors nbr_w under band {c['band_fit2']} and order {c['order2']}", again_w, got_w)
    if c["hand"] is not None:
        h = c["hand"]
        _, _, hand_id, hand_w = fit(d.up(h["P"]), d.up(h["fa"]), d.up(h["fb"]), c["band_fit2"], c["order2"], c["order2_items"])
        d.same("rk_rp3_neighbors nbr_id from the hand-made parts", hand_id, e["hand_id"])
        d.same("rk_rp3_neighbors nbr_w from the hand-made parts", hand_w, e["hand_w"])
    sid, nb = d.up(c["score_ids"], np.int32), len(c["score_ids"])
    mats = []
    for band in (c["band_score"], c["band_score2"]):
        o = d.out(nb * I, "float32")
        d.call("rk_rp3_scores", U, I, k, P(ids.full), P(w.full), ptr, idx, val, nb, sid, band, P(o.full))
        mats.append(d.read("rk_rp3_scores", o, (nb, I)))
    d.same("rk_rp3_scores", mats[0], e["scores"])
    d.same(f"rk_rp3_scores under band {c['band_score2']}", mats[1], mats[0])
    o = d.out(N_PAIRS, "float32")
    d.call("rk_rp3_pair_scores", I, U, k, P(ids.full), P(w.full), ptr, idx, val, d.up(c["pair_users"], np.int64),
           d.up(c["pair_items"], np.int64), N_PAIRS, P(o.full))
    got = d.read("rk_rp3_pair_scores", o)
    d.same("rk_rp3_pair_scores", got, e["pairs"])
    d.pairs_in_matrix("rk_rp3_pair_scores", got, mats[0], c["score_ids"])


def run_catchsync(c, dev):
    d = _Device(c, dev)
    e = expect_catchsync(c)
    U, I, P = c["U"], c["I"], d.P
    ptr, idx, _ = _csr_up(d)
    colptr_h, crow_h, _ = transpose(*csr(c))
    deg, reach_ = d.out(I, "int32"), d.out(I, "int32")
    d.call("rk_cs_features", U, I, ptr, d.up(colptr_h), d.up(crow_h), P(deg.full), P(reach_.full))
    d.same("rk_cs_features deg_item", d.read("deg_item", deg), e["deg_item"])
    d.same("rk_cs_features reach", d.read("reach", reach_), e["reach"])
    cell_of, count, info, st = d.out(I, "int32"), d.out(CR.MAX_CELLS, "int32"), d.out(4, "int64"), d.out(2, "int32")
    d.call("rk_cs_cells", I, P(deg.full), P(reach_.full), c["grid_bits"], P(cell_of.full), P(count.full), P(info.full), P(st.full))
    d.same("rk_cs_cells status", d.read("status", st), [0, -1])
    for name, o in (("cell_of", cell_of), ("cell_count", count), ("info", info)):
        d.same("rk_cs_cells " + name, d.read(name, o), e[name])
    M = max(int(e["info"][0]), 1)
    sums = []
    for n, form in enumerate([c["form"]] + [f for f in range(3) if f != c["form"]]):
        pair, back = d.out(U, "int64"), d.out(U, "int64")
        order = _order_up(d, c["order"], c["order_users"]) if n == 0 else _order_up(d, c["order2"], c["order2_users"])
        d.call("rk_cs_user_sums", U, ptr, idx, P(cell_of.full), P(count.full), M, form, order, P(pair.full), P(back.full))
        sums.append((pair, back, d.read("pair_num", pair), d.read("back_num", back), FORMS[form]))
    d.same(f"rk_cs_user_sums pair_num ({sums[0][4]} form)", sums[0][2], e["pair_num"])
    d.same(f"rk_cs_user_sums back_num ({sums[0][4]} form)", sums[0][3], e["back_num"])
    for other in sums[1:]:
        d.same(f"rk_cs_user_sums pair_num, {other[4]} form against {sums[0][4]}", other[2], sums[0][2])
        d.same(f"rk_cs_user_sums back_num, {other[4]} form against {sums[0][4]}", other[3], sums[0][3])
    score = d.out(U, "float32")
    d.call("rk_cs_scores", U, ptr, P(sums[0][0].full), P(sums[0][1].full), P(info.full), c["mode"], c["min_items"], P(score.full))
    d.same("rk_cs_scores", d.read("score", score), e["scores"])
    sel = d.out(c["m_select"], "int32")
    d.call("rk_knn_select", U, P(score.full), c["m_select"], 1, P(sel.full))
    d.same("rk_knn_select", d.read("order_out", sel), e["selected"])


RUN = {"neighbours": run_neighbours, "rp3": run_rp3, "catchsync": run_catchsync}


def run(seed=SEED, n_cases=None, leg="neighbours", dev=None):
    """One device pass over the cases 0 .. n_cases - 1 of a leg; raises Mismatch on the first difference."""
    import time

    import torch
    dev = torch.device("cuda:0") if dev is None else dev
    n_cases = N_CASES[leg] if n_cases is None else n_cases
    t0 = time.perf_counter()
    for index in range(n_cases):
        RUN[leg](case(seed, index), dev)
    torch.cuda.synchronize()
    print(f"{leg}: {n_cases} cases ok (seed {seed}) in {time.perf_counter() - t0:.1f} s, host side included")


if __name__ == "__main__":
    for leg_ in ([sys.argv[3]] if len(sys.argv) > 3 else LEGS):
        run(int(sys.argv[1]) if len(sys.argv) > 1 else SEED, int(sys.argv[2]) if len(sys.argv) > 2 else None, leg_)
