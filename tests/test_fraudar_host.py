"""CPU tests of the FraudarSelectUsers defender: the two restatements of the peel (tests/_fraudar_restate.py: a lazy-deletion
heap and an O(N^2) scan) against each other, the greedy guarantee by enumeration of every subset, the counts on synth `tiny`
with and without constructed attacks, the variants the definition rules out, n_blocks, and the registry / lazy-init / refusal
plumbing."""
import os

import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, defense, model, synth
from recad_amd.defense.fraudar_select_users import FraudarSelectUsers, check_config, weight_table
from recad_amd.defense.pca_select_users import flag_count
from recad_amd.utils import NotInstantiatedError
from tests import _fraudar_restate as R


def _csr(A):
    A = np.asarray(A) != 0
    return np.concatenate([[0], np.cumsum(A.sum(axis=1))]).astype(np.int64), np.nonzero(A)[1].astype(np.int64)


def _random(rng, max_u, max_i, min_size=1):
    """A random graph with empty rows and empty columns; the weight kind alternates with the draw."""
    U, I = int(rng.integers(min_size, max_u + 1)), int(rng.integers(min_size, max_i + 1))
    A = rng.random((U, I)) < rng.choice([0.1, 0.3, 0.6])
    A[rng.random(U) < 0.15] = False
    A[:, rng.random(I) < 0.15] = False
    ptr, idx = _csr(A)
    kind = ("log", "degree")[int(rng.integers(2))]
    return U, I, ptr, idx, R.weight_table(U, kind)[R.degrees(idx, I)], kind


# ------------------------------------------------------------------------------------------------- the restatement with itself
def test_heap_and_scan_agree_in_every_word():
    rng = np.random.default_rng(2016)
    seen_empty_row = seen_empty_col = 0
    for _ in range(200):
        U, I, ptr, idx, w, _ = _random(rng, 40, 40)
        a, b = R.peel(U, I, ptr, idx, w), R.peel_scan(U, I, ptr, idx, w)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3], (U, I)
        assert sorted(a[0].tolist()) == list(range(U + I)) and np.array_equal(a[0][a[1]], np.arange(U + I))
        seen_empty_row += bool((np.diff(ptr) == 0).any())
        seen_empty_col += bool((R.degrees(idx, I) == 0).any())
    assert seen_empty_row > 50 and seen_empty_col > 50


def test_weight_table():
    for U, off in ((300, 5.0), (7, 5.0), (50, 3.0), (1, 2.75)):
        want = R.weight_table(U, "log", off)
        assert np.array_equal(weight_table(U, "log", off), want) and want.dtype == np.uint32
        assert np.all(want >= 1) and np.all(want <= R.ONE) and np.all(np.diff(want.astype(np.int64)) < 0)
        d = np.arange(U + 1)
        assert np.max(np.abs(want / 2.0 ** 24 - 1.0 / np.log(d + off))) <= 2.0 ** -25 * (1 + 1e-9), "half a unit of 2^-24 per edge"
    assert np.array_equal(weight_table(9, "degree", 5.0), np.full(10, R.ONE, dtype=np.uint32))
    assert weight_table(3, "log", 1.5)[0] > R.ONE, "ln(d + log_offset) < 1: the device refuses this entry when an item meets it"
    assert weight_table(3, "log", 1.0 + 1e-12)[0] == 2 ** 32 - 1


def test_greedy_guarantee_by_enumeration():
    """g(S_t*) >= max_S g(S) / 2 over every non-empty subset of the nodes, 300 random graphs with U and I in 1..6."""
    rng = np.random.default_rng(7)
    worst = 1.0
    for _ in range(300):
        U, I, ptr, idx, w, _ = _random(rng, 6, 6)
        N = U + I
        _, step_of, _, (t, f, n) = R.peel(U, I, ptr, idx, w)
        assert R.g_of(U, I, ptr, idx, w, np.nonzero(step_of >= t)[0]) == (f, n)
        masks = np.arange(1, 1 << N, dtype=np.int64)
        inside = np.zeros(len(masks), dtype=np.int64)
        for u in range(U):
            for i in idx[ptr[u]:ptr[u + 1]]:
                inside += ((masks >> u) & 1) * ((masks >> (U + int(i))) & 1) * int(w[int(i)])
        size = np.zeros(len(masks), dtype=np.int64)
        for v in range(N):
            size += (masks >> v) & 1
        assert np.all(2 * f * size >= inside * n), (U, I)
        if inside.max() > 0:
            worst = min(worst, float(np.min((f / n) / np.maximum(inside / size, 1e-300))))
    print("worst g(S_t*) / max g(S):", worst)
    assert worst >= 0.5


# --------------------------------------------------------------------------------------------------------------- synth `tiny`
def _tiny_arrays():
    d = synth.make("tiny")
    ptr, idx = (np.asarray(a) for a in d["train"])
    return ptr[:301].astype(np.int64), idx[: ptr[300]].astype(np.int64), 300, 200


def planted(n_fake, n_items):
    """`tiny` plus n_fake users (ids 300...) who all rate the n_items least-rated items."""
    ptr, idx, U, I = _tiny_arrays()
    items = np.sort(np.argsort(R.degrees(idx, I), kind="stable")[:n_items])
    return (np.concatenate([ptr, ptr[-1] + n_items * np.arange(1, n_fake + 1)]), np.concatenate([idx] + [items] * n_fake), U + n_fake, I,
            items)


def test_tiny_block_and_the_textbook_greedy():
    ptr, idx, U, I = _tiny_arrays()
    w = R.weights(R.degrees(idx, I), "log", 5.0, U)
    _, step_of, _, (t, f, n) = R.peel(U, I, ptr, idx, w)
    users, items = R.block_of(step_of, t, U)
    assert (t, len(users), len(items), n) == (241, 111, 148, 259) and round(f / (n * 2.0 ** 24), 7) == 3.7337567
    tu, ti = R.textbook(U, I, ptr, idx)
    assert np.array_equal(tu, users) and np.array_equal(ti, items), "removal orders differ at tied priorities; the block does not"
    assert R.blocks(U, I, ptr, idx)[0]["density"] == f / (n * 2.0 ** 24)


def test_planted_40_by_40_is_the_block():
    ptr, idx, U, I, items = planted(40, 40)
    w = R.weights(R.degrees(idx, I), "log", 5.0, U)
    _, step_of, _, (t, _, n) = R.peel(U, I, ptr, idx, w)
    users, got_items = R.block_of(step_of, t, U)
    assert t == 460 and n == 80 and users.tolist() == list(range(300, 340)) and np.array_equal(got_items, items)
    assert R.flagged(U, I, ptr, idx) == list(range(300, 340))


def test_planted_50_by_20_block_and_count():
    """select="block" flags 162 users here: the natural core of a 10 %-dense toy set is denser than 50 x 20, and the block that
    holds the fake users holds it too.  FRAUDAR on such data, not a fault: select="count" flags exactly the 50."""
    ptr, idx, U, I, _ = planted(50, 20)
    block = R.flagged(U, I, ptr, idx)
    assert len(block) == 162 and set(range(300, 350)) <= set(block) and block == sorted(block)
    count = R.flagged(U, I, ptr, idx, select="count", m=flag_count(50, U))
    assert sorted(count) == list(range(300, 350))


def test_two_blocks():
    ptr, idx, U, I, items = planted(40, 40)
    b = R.blocks(U, I, ptr, idx, n_blocks=2)
    assert len(b) == 2 and b[0]["users"].tolist() == list(range(300, 340)) and np.array_equal(b[0]["items"], items) and b[0]["t_best"] == 460
    rest_ptr, rest_idx = R.drop_block(U, ptr, idx, b[0]["users"], b[0]["items"])
    assert len(rest_idx) == len(idx) - 1600 and np.all(np.diff(rest_ptr)[300:] == 0)
    fresh = R.blocks(U, I, rest_ptr, rest_idx)[0]
    assert all(np.array_equal(b[1][k], fresh[k]) for k in ("users", "items")) and all(b[1][k] == fresh[k] for k in ("t_best", "f_best", "n_best"))
    assert R.flagged(U, I, ptr, idx, n_blocks=2) == list(range(300, 340)) + b[1]["users"].tolist()
    assert R.blocks(U, I, np.zeros(U + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), n_blocks=3) == []
    one_edge = R.blocks(2, 2, np.array([0, 1, 1]), np.array([1]), n_blocks=4)
    assert len(one_edge) == 1 and one_edge[0]["users"].tolist() == [0] and one_edge[0]["items"].tolist() == [1], "a round without a block ends it"


# ------------------------------------------------------------------------------------------- variants the definition rules out
def test_mutations_are_rejected():
    rng = np.random.default_rng(99)
    changed = dict.fromkeys(("tie_high", "item_first", "latest", "charge_removed", "alive_degree"), 0)
    for _ in range(60):
        U, I, ptr, idx, w, kind = _random(rng, 12, 12, min_size=3)
        base = R.peel(U, I, ptr, idx, w)
        for name in ("tie_high", "item_first", "latest", "charge_removed"):
            got = R.peel(U, I, ptr, idx, w, **{name: True})
            changed[name] += (not np.array_equal(got[0], base[0])) or got[3] != base[3]
        alive = R.peel_scan(U, I, ptr, idx, w, alive_tab=R.weight_table(U, kind))
        changed["alive_degree"] += (not np.array_equal(alive[0], base[0])) or alive[3] != base[3]
    assert all(n > 0 for n in changed.values()), changed
    # the latest maximum on purpose: an empty graph has f_t / n_t = 0 throughout, two equal components repeat the first one's ratio
    empty = (np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64))
    assert R.peel(3, 2, *empty, [R.ONE] * 2)[3] == (0, 0, 5) and R.peel(3, 2, *empty, [R.ONE] * 2, latest=True)[3][0] == 4


# -------------------------------------------------------------------------------------------------------------------- plumbing
def _tiny():
    d = synth.make("tiny")
    return dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                               need_graph=False, device=torch.device("cpu"), seed=5)


def test_registry_defaults_and_lazy_init():
    assert model.factories["defender"]["FraudarSelectUsers"] is FraudarSelectUsers is defense.FraudarSelectUsers
    cfg = default.MODEL["defender"]["FraudarSelectUsers"]
    assert {k: cfg[k] for k in ("weight", "log_offset", "select", "n_blocks", "attack_num")} == {
        "weight": "log", "log_offset": 5.0, "select": "block", "n_blocks": 1, "attack_num": 50}
    names = {"rk_fd_init", "rk_fd_peel", "rk_fd_peel_ex"}
    assert names <= set(_lib.EXPORTS) and _lib.ABI_VERSION == 11
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "recad_hip.h")).read()
    assert all(f"int {n}(" in header for n in names) and "#define RK_ABI_VERSION 11" in header
    assert f"#define RK_FD_BAD_WEIGHT {R.BAD_WEIGHT}" in header and f"#define RK_FD_BAD_DEGREE {R.BAD_DEGREE}" in header
    assert _lib.RK_FD_MAX_NODES == R.MAX_NODES >= 1 << 17 and _lib.RK_FD_WEIGHT_ONE == R.ONE and set(_lib.RK_FD_RULES) == {R.BAD_WEIGHT, R.BAD_DEGREE}
    lazy = model.from_config("defender", "FraudarSelectUsers", attack_num=15, not_a_key=1)
    assert lazy.model_name == "FraudarSelectUsers"
    assert lazy._init_config["attack_num"] == 15 and lazy._init_config["log_offset"] == 5.0 and "not_a_key" not in lazy._init_config
    for call in (lambda: lazy.defense_step(), lambda: lazy.input_describe()):
        with pytest.raises(NotInstantiatedError):
            call()
    ds = _tiny()
    real = lazy.I(dataset=ds)
    assert real.I() is real and real.user_num == ds.n_users and real.item_num == ds.n_items
    cs = model.from_config("defender", "CatchSyncSelectUsers").I(dataset=ds)
    assert real.input_describe() == cs.input_describe() and real.output_describe() == cs.output_describe()
    assert real.reset(select="count")._init_config["select"] == "count"
    assert real.step_of is None and real.ranking is None and real.blocks is None and real.predLabels is None
    with pytest.raises(_lib.HipCallError):
        real.defense_step()      # CPU device: no fallback


@pytest.mark.parametrize("key,value", [("weight", "sqrt"), ("weight", None), ("select", "top"), ("select", 1), ("log_offset", 1.0),
                                       ("log_offset", 0.5), ("log_offset", float("inf")), ("log_offset", float("nan")),
                                       ("log_offset", "5"), ("log_offset", None), ("log_offset", True), ("n_blocks", 0), ("n_blocks", 9),
                                       ("n_blocks", True), ("n_blocks", 2.0), ("n_blocks", None)])
def test_host_side_refusals_need_no_library(monkeypatch, key, value):
    def no_library(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    d = model.from_config("defender", "FraudarSelectUsers", **{key: value}).I(dataset=_tiny())
    with pytest.raises(ValueError, match=key):
        d.defense_step()
    both = model.from_config("defender", "FraudarSelectUsers", n_blocks=2, select="count").I(dataset=_tiny())
    with pytest.raises(ValueError, match="n_blocks"):
        both.defense_step()
    nothing = model.from_config("defender", "FraudarSelectUsers").I(dataset=None)
    with pytest.raises(ValueError, match="dataset"):
        nothing.defense_step()
    check_config("log", 5.0, "block", 8)
    check_config("degree", 1.0001, "count", 1)
    check_config("log", np.float32(2.5), "block", np.int64(3))
