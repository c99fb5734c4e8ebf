"""What the seeded sweep of tests/tools/csr_kernel_sweep.py is worth, shown without a GPU: every generated case is inside every
entry's contract and rebuilds from (seed, index); over the very cases the GPU test runs the restatements reach the paths the
sweep is for (a tie at the cut, a band of more than 256 candidates, padding, several bands, every CatchSync form and mode, both
ways a neighbour row is gathered, equal and unequal cell counts); and each of ten wrong restatements, built here and never in
product code, changes the expected output of at least one case of its leg: the sweep can see that class of error."""
import collections
import functools

import numpy as np
import pytest

from tests import _catchsync_restate as CR
from tests import _itemknn_restate as IR
from tests import _knn_restate as K
from tests import _rp3_restate as PR
from tests.tools import csr_kernel_sweep as S


@functools.lru_cache(maxsize=None)
def _cases():
    return [S.case(S.SEED, i) for i in range(max(S.N_CASES.values()))]


def _leg_cases(leg):
    return _cases()[: S.N_CASES[leg]]


@functools.lru_cache(maxsize=None)
def _expected(leg):
    return [S.expected(c, leg) for c in _leg_cases(leg)]


def _bits(a):
    return S._bits(np.asarray(a))


def _differs(a, b):
    return any(not np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------ validity
def test_every_case_is_inside_every_contract():
    for c in _cases():
        U, I, ptr, idx, val = c["U"], c["I"], c["ptr"], c["idx"], c["val"]
        where = (c["seed"], c["index"])
        assert 1 <= U <= 300 and 1 <= I <= 700 and len(ptr) == U + 1 and ptr[0] == 0 and ptr[-1] == len(idx) == len(val), where
        assert ptr.dtype == np.int32 and idx.dtype == np.int32 and val.dtype == np.float32, where
        assert K.first_violation(ptr, idx, val, I) is None, where
        tp, ti, tv = S.transpose(ptr, idx, val, I)
        assert K.first_violation(tp, ti, tv, U) is None, where           # the transposed roles are a CSR under the same rules
        assert c["k"] in S.KS and all(c[b] in S.BANDS for b in ("band_fit", "band_fit2", "band_score", "band_score2")), where
        assert c["user_block"] in S.USER_BLOCKS and c["user_block2"] in S.USER_BLOCKS and c["normalize"] in (0, 1), where
        assert c["alpha"] in S.EXPONENTS and c["beta"] in S.EXPONENTS and 0 <= min(S.EXPONENTS) and max(S.EXPONENTS) <= 4, where
        assert 0 <= c["grid_bits"] <= 3 and c["form"] in (0, 1, 2) and c["mode"] in (0, 1, 2) and c["min_items"] in S.MIN_ITEMS, where
        assert 0 <= c["m_select"] <= U, where
        for name in ("order", "order2"):
            for side, n in (("users", U), ("items", I)):
                o = S.order_of(c[name], c[f"{name}_{side}"])
                assert o is None or np.array_equal(np.sort(o), np.arange(n)), where
        ids = c["user_ids"]
        assert ids.dtype == np.int32 and len(ids) >= 1 and ids.min() >= 0 and ids.max() < U, where       # rk_itemknn_scores checks none
        empty = np.nonzero(np.diff(ptr) == 0)[0]
        assert not len(empty) or np.isin(ids, empty).any(), where
        foreign = c["score_ids"][(c["score_ids"] < 0) | (c["score_ids"] >= U)]
        assert sorted(foreign.tolist()) == [-1, U, 2 ** 30] and set(c["score_ids"].tolist()) - set(foreign.tolist()) == set(ids.tolist()), where
        pu, pi = c["pair_users"], c["pair_items"]
        assert pu.dtype == np.int64 and pi.dtype == np.int64 and len(pu) == len(pi) == S.N_PAIRS, where
        ok = (pu >= 0) & (pu < U) & (pi >= 0) & (pi < I)
        assert 0 < (~ok).sum() <= 8 and np.isin(pu[ok], ids).all(), where   # in-range pairs are entries of the scored matrix
        if c["hand"] is not None:
            h = c["hand"]
            assert h["P"].dtype == np.int64 and len(h["P"]) == len(idx) and (len(idx) == 0 or h["P"].min() >= 1), where
            assert h["P"].sum() < 2 ** 62 and np.all(h["fa"] > 0) and np.all(h["fb"] > 0) and len(h["fa"]) == len(h["fb"]) == I, where
    repeats = [len(set(c["user_ids"].tolist())) < len(c["user_ids"]) for c in _cases()]
    assert any(repeats) and not all(repeats), "blocks with and without a repeated user"


def test_a_case_rebuilds_from_seed_and_index():
    for c in _cases()[::7]:
        again = S.case(c["seed"], c["index"])
        assert again.keys() == c.keys()
        for name, v in c.items():
            if name == "hand":
                assert (v is None) == (again[name] is None) and (v is None or all(np.array_equal(v[x], again[name][x]) for x in v))
            else:
                assert np.array_equal(v, again[name]), name
    other = S.case(S.SEED + 1, 0)
    assert other["U"] != _cases()[0]["U"] or other["I"] != _cases()[0]["I"] or not np.array_equal(other["idx"], _cases()[0]["idx"])


def test_the_comparison_sees_one_bit_and_says_where():
    want = np.array([[0.0, 0.5, 1.0], [2.0, 3.0, 4.0]], dtype=np.float32)
    assert S.difference(want.copy(), want) is None and S.difference(np.arange(5, dtype=np.int32), list(range(5))) is None
    got = want.copy()
    got[0, 0], got[1, 2] = -0.0, np.nextafter(np.float32(4), np.float32(5))
    assert "2 of 6 elements differ, first at [[0, 0], [1, 2]]" in S.difference(got, want)
    got = want.copy()
    got[1, 1] = np.nan                                                 # an element the kernel never wrote
    assert "[[1, 1]]" in S.difference(got, want)
    assert "[[3]]" in S.difference(np.array([0, 1, 2, -777, 4]), np.arange(5))
    assert "shape" in S.difference(want[:1], want) and "type" in S.difference(want.astype(np.float64), want)
    with pytest.raises(AssertionError, match="sentinel"):
        S.difference(want, got)
    c = _cases()[3]
    report = S.params(c)
    assert report["seed"] == S.SEED and report["index"] == 3 and report["k"] == c["k"] and report["nnz"] == len(c["idx"])
    assert not any(isinstance(v, np.ndarray) for v in report.values())


def test_case_counts_are_the_measured_ones():
    """N_CASES is what the tool's docstring reports the host times for."""
    for leg, n in S.N_CASES.items():
        assert f"{leg:<11}{n:>4} cases" in S.__doc__, leg


# ------------------------------------------------------------------------------------------------------------------ reach
@functools.lru_cache(maxsize=None)
def _reach(leg):
    counts = collections.Counter()
    for c in _leg_cases(leg):
        counts.update(name for name, hit in S.reach(c, leg).items() if hit)
    print(f"reach of the {leg} leg over {S.N_CASES[leg]} cases: {dict(sorted(counts.items()))}")
    return counts


@pytest.mark.parametrize("leg", ["neighbours", "rp3"])
def test_reach_of_the_neighbour_lists(leg):
    n, got = S.N_CASES[leg], _reach(leg)
    assert 2 * got["tie_at_cut"] >= n, "at least half the cases have a tie exactly at the cut"
    assert 10 * got["over_256"] >= n, "at least 1 in 10 has a band with more than 256 candidates"
    assert 10 * got["padded"] >= n, "at least 1 in 10 has a padded list"
    assert 4 * got["bands"] >= n, "at least 1 in 4 has more than one band"
    if leg == "neighbours":
        assert got["row_searched"] >= 1 and got["row_strided"] >= 1, "both ways rk_userknn_scores gathers a neighbour row"


def test_reach_of_the_catchsync_leg():
    got = _reach("catchsync")
    for name in ["form_" + f for f in S.FORMS] + ["mode_" + m for m in CR.MODES]:
        assert got[name] >= 10, name
    assert got["cells_unequal"] >= 10 and got["cells_all_equal"] >= 1


# ------------------------------------------------------------------------------------------------------------------ power
def _item_tables(c, tie_high=False, keep_self=False, swapped=False, k_full=False):
    """IR.neighbours with one rule of the definition changed at a time."""
    D, W = IR.similarities(K.dense(*S.csr(c)))
    if swapped:                                                        # ((float) d * r_j) * r_i: d is symmetric
        W = np.ascontiguousarray(W.T)
    I, k = c["I"], c["k"]
    k_eff = min(k, I if k_full else I - 1)
    nbr_id, nbr_w = np.full((k, I), -1, dtype=np.int32), np.zeros((k, I), dtype=np.float32)
    for i in range(I):
        cand = np.nonzero(D[i] > 0)[0]
        if not keep_self:
            cand = cand[cand != i]
        cand = cand[np.lexsort((-cand if tie_high else cand, -W[i, cand].astype(np.float64)))][:k_eff]
        nbr_id[: len(cand), i], nbr_w[: len(cand), i] = cand, W[i, cand]
    return nbr_id, nbr_w


def _rows(A, nbr_id, nbr_w, users, items=None, fused=False, descending=False):
    """IR._rows with the term fused into the add (formed in float64, rounded once) or the slots taken from the last."""
    users = np.asarray(users, dtype=np.int64)
    Q = A[users].astype(np.float32)
    n, I = Q.shape
    cols = np.arange(I) if items is None else np.asarray(items, dtype=np.int64)
    s = np.zeros((n, I) if items is None else n, dtype=np.float32)
    slots = range(nbr_id.shape[0])
    for t in (reversed(slots) if descending else slots):
        ids, w = nbr_id[t, cols], nbr_w[t, cols]
        q = Q[:, np.maximum(ids, 0)] if items is None else Q[np.arange(n), np.maximum(ids, 0)]
        if fused:
            new = (s.astype(np.float64) + w.astype(np.float64) * q.astype(np.float64)).astype(np.float32)
        else:
            new = (s + (w * q).astype(np.float32)).astype(np.float32)
        s = np.where(ids >= 0, new, s)
    return s


def _degsim_k_full(c):
    """K.degsim with k_eff = min(k, U): the mean's divisor counts the user itself."""
    A = K.dense(*S.csr(c))
    U, r, k = A.shape[0], K.rnorm(A), c["k"]
    W = ((A @ A.T).astype(np.float32) * r[:, None]) * r[None, :]
    k_eff = min(k, U)
    topw, out = np.zeros((U, k), dtype=np.float32), np.zeros(U, dtype=np.float32)
    for u in range(U):
        top = -np.sort(-np.delete(W[u], u), kind="stable")[:k_eff]
        topw[u, : len(top)] = top
        out[u] = K.mean_of(topw[u], k_eff)
    return topw, out


def _bucket_one_lower(x, s):
    x = int(x)
    e = x.bit_length() - 1
    sh = e - s - 1
    return e * (1 << s) + ((x >> sh if sh >= 0 else x << -sh) & ((1 << s) - 1))


def _weights_other_order(S_, fa, fb):
    """PR.weights as (S * (fa_i * fb_j)) * 2^-40."""
    return ((S_.astype(np.float64) * (fa[:, None] * fb[None, :])) * (1.0 / PR.SCALE)).astype(np.float32)


def patch_one_rule(leg, monkeypatch):
    """One wrong rule per leg, patched into the restatements: what tests/test_csr_kernel_sweep_gpu.py feeds the device pass to see
    it report a difference."""
    if leg == "neighbours":
        monkeypatch.setattr(IR, "_rows", functools.partial(_rows, fused=True))
    elif leg == "rp3":
        monkeypatch.setattr(PR, "weights", _weights_other_order)
    else:
        monkeypatch.setattr(CR, "bucket", _bucket_one_lower)


_USER_SUMS = CR.user_sums


def _user_sums_distinct(ptr, idx, cell_of, cell_count, M):
    pair, back = _USER_SUMS(ptr, idx, cell_of, cell_count, M)
    for u in range(len(ptr) - 1):
        cells = np.asarray(cell_of, dtype=np.int64)[np.asarray(idx[ptr[u]:ptr[u + 1]], dtype=np.int64)]
        cells = np.unique(cells[(cells >= 0) & (cells < M)])
        back[u] = int(np.asarray(cell_count, dtype=np.int64)[cells].sum())
    return pair, back


def _mutant(number, c, e, monkeypatch):
    """(expected outputs of case c under mutant `number`, the true ones)."""
    if number in (1, 2, 3):
        return _item_tables(c, tie_high=number == 1, keep_self=number == 2, swapped=number == 3), (e["item_id"], e["item_w"])
    if number in (4, 5):
        monkeypatch.setattr(IR, "_rows", functools.partial(_rows, fused=number == 4, descending=number == 5))
        return [IR.scores(*S.csr(c), e["item_id"], e["item_w"], c["user_ids"])], [e["item_scores"]]
    if number == 6:
        return _item_tables(c, k_full=True) + _degsim_k_full(c), (e["item_id"], e["item_w"], e["topw"], e["degsim"])
    if number == 7:
        q = c["val"].astype(np.int64)
        r = e["r"][np.repeat(np.arange(c["U"]), np.diff(c["ptr"]))]
        return [np.rint(PR.SCALE * PR._power(q.astype(np.float64) / r.astype(np.float64), c["alpha"])).astype(np.int64)], [e["P"]]
    if number == 8:
        monkeypatch.setattr(PR, "weights", _weights_other_order)
        got = list(S.rp3_tables(c, e["P"], e["fa"], e["fb"]))
        want = [e["nbr_id"], e["nbr_w"]]
        if c["hand"] is not None:
            got += S.rp3_tables(c, c["hand"]["P"], c["hand"]["fa"], c["hand"]["fb"])
            want += [e["hand_id"], e["hand_w"]]
        return got, want
    if number == 9:
        monkeypatch.setattr(CR, "bucket", _bucket_one_lower)
    else:
        monkeypatch.setattr(CR, "user_sums", _user_sums_distinct)
    got = S.expect_catchsync(c)
    return [got[name] for name in sorted(got)], [e[name] for name in sorted(e)]


MUTANTS = {1: ("neighbours", "ties go to the higher id"), 2: ("neighbours", "the item itself stays a candidate"),
           3: ("neighbours", "w = ((float) d * r_j) * r_i"), 4: ("neighbours", "the score term is one fused multiply-add"),
           5: ("neighbours", "scores summed in descending slot order"), 6: ("neighbours", "k_eff = min(k, I)"),
           7: ("rp3", "P without the max(1, .) floor"), 8: ("rp3", "the weight multiplied as S * (fa * fb)"),
           9: ("catchsync", "the bucket takes the s bits one position lower"), 10: ("catchsync", "back_num counts distinct cells")}


def test_the_unswitched_variants_are_the_restatements():
    """The mutants differ from the restatements by their one switch alone."""
    for c, e in list(zip(_leg_cases("neighbours"), _expected("neighbours")))[:12]:
        assert not _differs(_item_tables(c), (e["item_id"], e["item_w"]))
        A = K.dense(*S.csr(c))
        assert not _differs([_rows(A, e["item_id"], e["item_w"], c["user_ids"])], [e["item_scores"]])
    for x in list(range(1, 70)) + [127, 128, 1000, 2 ** 31 - 1]:
        assert _bucket_one_lower(x, 0) == CR.bucket(x, 0) and all(_bucket_one_lower(x, s) >> s == CR.bucket(x, s) >> s for s in (1, 2, 3))


@pytest.mark.parametrize("number", sorted(MUTANTS))
def test_each_mutant_moves_a_case(number, monkeypatch):
    leg, what = MUTANTS[number]
    moved = []
    for c, e in zip(_leg_cases(leg), _expected(leg)):
        with monkeypatch.context() as m:
            got, want = _mutant(number, c, e, m)
        if _differs(got, want):
            moved.append(c["index"])
    print(f"mutant {number} ({what}) moves {len(moved)} of {S.N_CASES[leg]} cases of the {leg} leg, the first {moved[:5]}")
    assert moved, f"the sweep cannot see: {what}"
