"""CPU tests of the CatchSyncSelectUsers defender: bucket against bit-length arithmetic, the numpy restatement of the
definition (tests/_catchsync_restate.py) against the literal definition in exact rationals, the variants the definition rules
out, the edge cases, a constructed attack flagged entirely, the detection probe on synthetic data, and the registry /
lazy-init / refusal / workflow plumbing."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, defense, model, synth, workflow
from recad_amd.defense.catchsync_select_users import CatchSyncSelectUsers, check_config
from recad_amd.defense.pca_select_users import flag_count
from recad_amd.evaluate import detection_quality
from recad_amd.utils import NotInstantiatedError
from tests import _catchsync_probe as Q
from tests import _catchsync_restate as R


def _csr(A):
    A = np.asarray(A) != 0
    return np.concatenate([[0], np.cumsum(A.sum(axis=1))]).astype(np.int64), np.nonzero(A)[1].astype(np.int64), A.shape[1]


def _random(U, I, density, seed):
    """Item popularity spread over two decades, so that several cells exist."""
    rng = np.random.default_rng(seed)
    return rng.random((U, I)) < 2 * density * rng.random(I)[None, :]


# --------------------------------------------------------------------------------------------------------------------- bucket
def _bucket_by_bit_length(x, s):
    e = x.bit_length() - 1
    return ((x << s) >> e) - (1 << s) + (e << s)


def test_bucket():
    for s in range(4):
        xs = {1, 2, 3, 2 ** 31 - 1}
        for e in range(31):
            for m in range(1 << s):
                num = (1 << e) * ((1 << s) + m)
                if num % (1 << s) == 0:                   # the boundary x = 2^e (2^s + m) / 2^s where it is an integer
                    xs.update({(num >> s) - 1, num >> s, (num >> s) + 1})
        xs = sorted(x for x in xs if 1 <= x <= 2 ** 31 - 1)
        got = [R.bucket(x, s) for x in xs]
        assert got == [_bucket_by_bit_length(x, s) for x in xs]
        assert got == sorted(got) and got[0] == 0 and got[-1] == 30 * (1 << s) + (1 << s) - 1 < 256      # monotone, one byte
        for e in range(s, 31):
            for m in range(1 << s):
                lo = ((1 << s) + m) << (e - s)
                assert R.bucket(lo, s) == e * (1 << s) + m and (e == s and m == 0 or R.bucket(lo - 1, s) == e * (1 << s) + m - 1)
    assert [R.bucket(x, 1) for x in (1, 2, 3, 4, 5, 6, 7, 8)] == [0, 2, 3, 4, 4, 5, 5, 6]
    assert [R.bucket(x, 3) for x in (1, 3, 5)] == [0, 12, 18], "the missing low bits are zero-filled"


# --------------------------------------------------------------------------------------------- the literal definition, exactly
def _literal(ptr, idx, I, s):
    """cells as sorted (bucket(deg), bucket(reach)) tuples, and per user the three scores as exact rationals (None for d < 2)."""
    U = len(ptr) - 1
    rows = [set(idx[ptr[u]:ptr[u + 1]].tolist()) for u in range(U)]
    deg = [sum(i in r for r in rows) for i in range(I)]
    reach = [sum(len(r) for r in rows if i in r) for i in range(I)]
    key = {i: (_bucket_by_bit_length(deg[i], s), _bucket_by_bit_length(reach[i], s)) for i in range(I) if deg[i]}
    cells = sorted(set(key.values()))
    cell = {i: cells.index(k) for i, k in key.items()}
    M, N = len(cells), len(key)
    n_c = [sum(1 for c in cell.values() if c == j) for j in range(M)]
    s_b = Fraction(sum(c * c for c in n_c), N * N)
    out = []
    for r in rows:
        d = len(r)
        if d < 2:
            out.append(None)
            continue
        sync = Fraction(sum(cell[v] == cell[w] for v in r for w in r if v != w), d * (d - 1))
        normality = Fraction(sum(cell[v] == cell[w] for v in r for w in key), d * N)
        p = [Fraction(sum(1 for v in r if cell[v] == j), d) for j in range(M)]
        assert sum(p) == 1 and sum(pc * Fraction(nc, N) for pc, nc in zip(p, n_c)) == normality
        sy = sum(pc * pc for pc in p)
        s_min = Fraction(1, M) if len(set(n_c)) == 1 else (M * normality * normality - 2 * normality + s_b) / (M * s_b - 1)
        out.append((sync, normality, sy - s_min))
    return cell, M, out


@pytest.mark.parametrize("U,I,density,s", [(40, 30, 0.3, 1), (120, 60, 0.2, 0), (300, 120, 0.15, 2), (90, 100, 0.1, 3)])
def test_restatement_equals_the_literal_definition(U, I, density, s):
    """sync and normality are one correctly rounded fp64 division of exact integers, so they equal the rounded rationals; the
    residual is within 8 * 2^-53 of its rational before the fp32 rounding, and never below zero (the theorem)."""
    ptr, idx, _ = _csr(_random(U, I, density, U + s))
    cell, M, exact = _literal(ptr, idx, I, s)
    got = {m: R.run(ptr, idx, I, m, s, 2) for m in R.MODES}
    r = got["sync"]
    assert r["info"][0] == M and all(r["cell_of"][i] == cell.get(i, -1) for i in range(I))
    d = np.diff(ptr)
    assert sum(e is not None for e in exact) > U // 2
    for u, e in enumerate(exact):
        if e is None:
            assert all(got[m]["scores"][u] == -1 for m in R.MODES) and d[u] < 2
            continue
        assert got["sync"]["scores"][u] == np.float32(float(e[0])) and got["normality"]["scores"][u] == np.float32(float(e[1]))
        f64 = R.score_f64(d[u], r["pair_num"][u], r["back_num"][u], r["info"], "residual")
        assert abs(Fraction(f64) - e[2]) <= Fraction(8, 2 ** 53), float(abs(Fraction(f64) - e[2])) * 2 ** 53
        assert e[2] >= 0 and f64 >= -1e-12 and got["residual"]["scores"][u] == np.float32(f64)


def test_residual_is_zero_at_the_background_shares():
    """A user who holds every rated item has cell shares N_c / N: s = n = s_b and s_min(s_b) = s_b."""
    A = _random(60, 40, 0.25, 5)
    A[7] = A.any(axis=0)
    ptr, idx, I = _csr(A)
    r = R.run(ptr, idx, I, "residual", 1, 2)
    M, N, SB, all_equal = r["info"]
    assert not all_equal and r["pair_num"][7] == SB and r["back_num"][7] == SB and ptr[8] - ptr[7] == N
    assert abs(R.score_f64(N, SB, SB, r["info"], "residual")) <= 8 * 2.0 ** -53
    assert R.run(ptr, idx, I, "normality", 1, 2)["scores"][7] == np.float32(SB / (N * N))


# ------------------------------------------------------------------------------------------- variants the definition rules out
def test_mutations_are_rejected():
    """One graph: 30 x 24 random plus two unrated items (columns 24, 25), a user with one item and an empty user."""
    A = np.zeros((32, 26), dtype=bool)
    A[:30, :24] = _random(30, 24, 0.3, 2)
    A[30, 3] = True
    ptr, idx, I = _csr(A)
    s, min_items = 1, 4
    base = R.run(ptr, idx, I, "sync", s, min_items)
    d = np.diff(ptr)
    M, N, SB, all_equal = base["info"]
    elig = d >= min_items
    assert elig.sum() > 10 and N == 24 < I and not all_equal
    pair, back = base["pair_num"], base["back_num"]
    # self pairs counted in sync
    with_self = np.array([np.float32(pair[u] / (d[u] * d[u])) for u in np.nonzero(elig)[0]])
    assert np.any(with_self != base["scores"][elig])
    # unrated items counted in N; normality divided by I
    norm = R.scores(ptr, pair, back, base["info"], "normality", min_items)
    assert np.any(R.scores(ptr, pair, back, (M, I, SB, 0), "normality", min_items)[elig] != norm[elig])
    assert np.any(np.array([np.float32(back[u] / (d[u] * I)) for u in np.nonzero(elig)[0]]) != norm[elig])
    # empty cells counted in M: the whole grid between the smallest and the largest bucket of either feature
    bd = [R.bucket(x, s) for x in base["deg_item"] if x]
    br = [R.bucket(x, s) for x in base["reach"] if x]
    grid = (max(bd) - min(bd) + 1) * (max(br) - min(br) + 1)
    res = R.scores(ptr, pair, back, base["info"], "residual", min_items)
    assert grid > M and np.any(R.scores(ptr, pair, back, (grid, N, SB, 0), "residual", min_items)[elig] != res[elig])
    # reach summed over the item's own degree instead of its users' row lengths (deg_i once per user of the column: deg_i^2)
    assert np.any(R.cells(base["deg_item"], base["deg_item"] ** 2, s)[0] != base["cell_of"])
    # buckets without the sub-octave bit at s = 1
    assert np.any(R.cells(base["deg_item"], base["reach"], 0)[0] != base["cell_of"]) and R.cells(base["deg_item"], base["reach"], 0)[2][0] < M
    # the two key halves swapped in the ranking: the same partition, other cell numbers
    swapped = R.cells(base["reach"], base["deg_item"], s)
    assert swapped[2] == base["info"] and np.any(swapped[0] != base["cell_of"])
    # ineligible users scored 0 instead of -1; smallest-first selection
    assert np.all(base["scores"][~elig] == -1) and (~elig).sum() >= 2 and np.all(base["scores"][elig] >= 0)
    m = 5
    top = R.select(base["scores"], m)
    smallest = np.lexsort((np.arange(len(d)), base["scores"]))[:m].tolist()
    assert top != smallest and all(elig[u] for u in top) and not any(elig[u] for u in smallest[:2])
    zeroed = np.where(elig, base["scores"], np.float32(0))
    assert R.select(zeroed, len(d))[-1] != R.select(base["scores"], len(d))[-1] or np.any(zeroed != base["scores"])


# ------------------------------------------------------------------------------------------------------------------ edge cases
def test_equal_cells_and_single_cell():
    """Every user rates every item: one cell, s_min = 1 / M = 1, residual 0, no division by zero (Python would raise).  Two
    blocks of four items with different degrees: two cells of equal size, the same branch."""
    ptr, idx, I = _csr(np.ones((6, 5)))
    for mode, want in (("sync", 1.0), ("normality", 1.0), ("residual", 0.0)):
        r = R.run(ptr, idx, I, mode, 2, 2)
        assert r["info"] == (1, 5, 25, 1) and r["scores"].tolist() == [want] * 6
    A = np.zeros((12, 8))
    A[:, :4] = 1
    A[:2, 4:] = 1
    ptr, idx, I = _csr(A)
    r = R.run(ptr, idx, I, "residual", 0, 2)
    assert r["info"] == (2, 8, 32, 1)
    assert r["scores"].tolist() == [0.0, 0.0] + [0.5] * 10, "half and half is the background; all in one cell is 1 - 1/2"
    with pytest.raises(ZeroDivisionError):
        R.score_f64(4, 16, 16, (2, 8, 32, 0), "residual")      # what the all_equal branch is there for


def test_full_user_empty_users_and_unreachable_min_items():
    A = _random(50, 30, 0.3, 9)
    A[0] = A[20] = A[49] = False
    A[11] = True
    ptr, idx, I = _csr(A)
    r = R.run(ptr, idx, I, "sync", 1, 2)
    M, N, SB, _ = r["info"]
    assert N == I == 30 and r["pair_num"][11] == SB and r["back_num"][11] == SB
    assert r["scores"][11] == np.float32((SB - N) / (N * (N - 1)))
    assert r["scores"][[0, 20, 49]].tolist() == [-1.0] * 3 and r["pair_num"][[0, 20, 49]].tolist() == [0] * 3
    none = R.run(ptr, idx, I, "residual", 1, 31)
    assert np.all(none["scores"] == -1) and R.select(none["scores"], 7) == list(range(7)), "flags go to the lowest ids"
    empty = R.run(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64), 5, "sync", 1, 2)
    assert empty["info"] == (0, 0, 0, 1) and np.all(empty["scores"] == -1) and np.all(empty["cell_of"] == -1)


def test_restated_refusals():
    assert R.cells([3, -1, 2, -5], [4, 4, 4, 4], 1) == ("refused", R.BAD_FEATURE, 1)
    assert R.cells([3, 1, 2], [4, 4, 0], 1) == ("refused", R.BAD_FEATURE, 2)
    assert R.cells([0, 0], [0, 7], 1)[2] == (0, 0, 0, 1), "an unrated item's reach is not read"
    deg = [1, 2, 4, 8]
    assert R.cells(deg, [1, 1, 1, 1], 0, cap=3) == ("refused", R.TOO_MANY_CELLS, 3)
    assert R.cells(deg[::-1], [1, 1, 1, 1], 0, cap=3) == ("refused", R.TOO_MANY_CELLS, 0)
    assert R.cells(deg, [1, 1, 1, 1], 0, cap=4)[2] == (4, 4, 4, 1)


# ----------------------------------------------------------------------------------------------------- a constructed attack
def _tiny_arrays():
    d = synth.make("tiny")
    ptr, idx = (np.asarray(a) for a in d["train"])
    return ptr[:301].astype(np.int64), idx[: ptr[300]].astype(np.int64), 300, 200


def one_cell_attack(n_fake=10, n_items=20, seed=0):
    """How the set was chosen: the restatement runs on the clean `tiny` graph at grid_bits = 1; its largest cell holds 36 of
    the 200 items; every fake profile is 20 of those 36 (numpy's default_rng(0), one permutation per profile).  The injection
    itself moves degrees and reaches, so the choice is checked by running the restatement on the poisoned graph."""
    ptr, idx, U, I = _tiny_arrays()
    clean = R.run(ptr, idx, I, "sync", 1, 20)
    items = np.nonzero(clean["cell_of"] == int(np.argmax(clean["cell_count"])))[0]
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.permutation(items)[:n_items]) for _ in range(n_fake)]
    return np.concatenate([ptr, ptr[-1] + n_items * np.arange(1, n_fake + 1)]), np.concatenate([idx] + rows), U, I


def test_constructed_attack_is_flagged_entirely():
    ptr, idx, U, I = one_cell_attack()
    m = flag_count(10, U + 10)
    for mode, gap in (("sync", 0.08), ("residual", 0.02)):
        r = R.run(ptr, idx, I, mode, 1, 20)
        assert r["scores"][U:].min() - r["scores"][:U].max() > gap, (mode, r["scores"][U:].min(), r["scores"][:U].max())
        flagged = R.select(r["scores"], m)
        assert sorted(flagged) == list(range(U, U + 10)) and detection_quality(flagged, U, U + 10)["f1"] == 1.0


# ------------------------------------------------------------------------------------------------- the probe on synthetic data
def test_probe_counts_are_computed():
    """The counts of DESIGN.md section 17 at the default setting (grid_bits 1, min_items 20), every profile item an edge.
    Nothing is asserted about them beyond being counts: they describe synthetic data and are no claim about real data
    (scripts/cs_detection_probe.py prints the whole table, DegSim included)."""
    base = Q.clean()
    for kind in Q.ATTACKERS:
        ptr, idx, U, I = Q.poisoned(kind, "all", base)
        assert len(ptr) == U + Q.N_FAKE + 1 and np.all(np.diff(ptr)[U:] >= Q.FILLERS + 1)
        hits = Q.catchsync_hits(ptr, idx, U, I, 1, 20)
        print(kind, hits)
        assert set(hits) == set(R.MODES) and all(isinstance(h, int) and 0 <= h <= Q.N_FAKE for h in hits.values())


# -------------------------------------------------------------------------------------------------------------------- plumbing
def _tiny():
    d = synth.make("tiny")
    return dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                               need_graph=False, device=torch.device("cpu"), seed=5)


def test_registry_defaults_and_lazy_init():
    assert model.factories["defender"]["CatchSyncSelectUsers"] is CatchSyncSelectUsers is defense.CatchSyncSelectUsers
    cfg = default.MODEL["defender"]["CatchSyncSelectUsers"]
    assert {k: cfg[k] for k in ("score", "grid_bits", "min_items", "attack_num", "schedule", "form")} == {
        "score": "sync", "grid_bits": 1, "min_items": 20, "attack_num": 50, "schedule": "work", "form": None}
    assert {"rk_cs_features", "rk_cs_cells", "rk_cs_user_sums", "rk_cs_scores"} <= set(_lib.EXPORTS) and _lib.ABI_VERSION == 11
    assert _lib.RK_CS_MAX_CELLS == R.MAX_CELLS and set(_lib.RK_CS_RULES) == {R.BAD_FEATURE, R.TOO_MANY_CELLS}
    lazy = model.from_config("defender", "CatchSyncSelectUsers", attack_num=15, not_a_key=1)
    assert lazy.model_name == "CatchSyncSelectUsers"
    assert lazy._init_config["attack_num"] == 15 and lazy._init_config["min_items"] == 20 and "not_a_key" not in lazy._init_config
    for call in (lambda: lazy.defense_step(), lambda: lazy.input_describe()):
        with pytest.raises(NotInstantiatedError):
            call()
    ds = _tiny()
    real = lazy.I(dataset=ds)
    assert real.I() is real and real.user_num == ds.n_users and real.item_num == ds.n_items
    knn = model.from_config("defender", "KnnSelectUsers").I(dataset=ds)
    assert real.input_describe() == knn.input_describe() and real.output_describe() == knn.output_describe()
    assert real.reset(min_items=7)._init_config["min_items"] == 7
    assert real.scores is None and real.ranking is None and real.n_cells is None
    with pytest.raises(_lib.HipCallError):
        real.defense_step()      # CPU device: no fallback


@pytest.mark.parametrize("key,value", [("score", "sum"), ("score", None), ("grid_bits", 4), ("grid_bits", -1), ("grid_bits", 1.5),
                                       ("grid_bits", None), ("min_items", 1), ("min_items", 0), ("min_items", 2.5),
                                       ("min_items", None), ("schedule", "random"), ("form", "auto"), ("form", 1)])
def test_host_side_refusals_need_no_library(monkeypatch, key, value):
    def no_library(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    d = model.from_config("defender", "CatchSyncSelectUsers", **{key: value}).I(dataset=_tiny())
    with pytest.raises(ValueError, match=key):
        d.defense_step()
    check_config("residual", 3, 2, "natural", "workgroup")
    check_config("sync", 0, 1000, "work", None)
    check_config("normality", np.int64(2), np.int32(20), "work", "wave")


def test_detection_quality_through_a_defense_run():
    """workflow.Defense with a stub victim and a stub defender that answers what the restatement flags on the poisoned data."""
    from tests.test_host_logic import _StubVictim

    class Stub:
        def I(self, **kw):
            return self

        def to(self, device):
            return self

        def input_describe(self):
            return {"defense_step": {"dataset": None}}

        def defense_step(self, dataset=None):
            ptr, idx = dataset.train_csr_sorted()
            U, I = dataset.n_users, dataset.n_items
            r = R.run(np.asarray(ptr)[: U + 1], np.asarray(idx)[: int(ptr[U])], I, "sync", 1, 4)
            return R.select(r["scores"], flag_count(10, U))

    ds = _tiny()
    wf = workflow.from_config("defense", victim_data=ds, attack_data=None, victim=_StubVictim(),
                              attacker=workflow.RandomAttack(ds.n_items, attack_num=10, filler_num=5, seed=1),
                              defender=Stub(), rec_epoch=1, attack_epoch=0, device=torch.device("cpu"))
    res = wf.execute()
    m = flag_count(10, 310)
    assert set(res) == {"attacked", "defended", "n_flagged"} and res["n_flagged"] == m
    assert wf.fake_dataset.n_users == ds.n_users + 10
    assert wf.detection["n_flagged"] == m and wf.detection["n_fake"] == 10
    assert wf.detection["precision"] == wf.detection["true_positives"] / m
