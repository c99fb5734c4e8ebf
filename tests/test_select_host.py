"""CPU tests of the selection restatement (tests/_select_restate.py) that tests/test_score_select_forms_gpu.py holds the kernels
to: on every finite row of the case tables select_row is orc.topk_row bit for bit, six planted faults are each caught by a
named case, the bias order is the oracle's and no other, and the dispatch tables still say what the source says and are covered
by the cases."""
import os

import numpy as np
import pytest

from oracle import oracle as orc

from . import _select_restate as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_row(scores, seen, K, targets):
    """orc.topk_row with its list scores folded (-0.0 -> +0.0): the one place where the kernels' lists and the oracle's differ in
    bits on finite rows -- the oracle copies the score, the kernels return key_score(score_key(s)).  Target scores are copies in
    both and are compared unfolded."""
    ids, sc, ts, tr = orc.topk_row(scores, seen, K, targets)
    return ids, S.fold_zero(sc), ts, tr


def _rows():
    for c in S.SEL_CASES:
        yield from S.sel_rows(S.sel_case(*c))


@pytest.mark.parametrize("c", S.SEL_CASES, ids=S.sel_id)
def test_select_row_is_the_oracle_on_finite_rows(c):
    case = S.sel_case(*c)
    for name, scores, seen, K, targets in S.sel_rows(case):
        assert np.isfinite(scores).all()
        assert S.same_row(S.select_row(scores, seen, K, targets), _oracle_row(scores, seen, K, targets)), name


def test_scoring_cases_select_like_the_oracle():
    """the finite scoring cases (reference scores from the restated chain): instantiation, edge and bias cases"""
    cases = [S.inst_case(i) for i in S.PANEL_INSTANTIATIONS[::5]] + [S.edge_case(n) for n in (17, 1921, 3841)] + [S.edge_case(3841, 1), S.bias_case()]
    for c in cases:
        for b, u in enumerate(c["user_ids"]):
            seen = c["seen_lists"][int(u)]
            assert S.same_row(S.select_row(c["ref"][b], seen, c["K"], c["targets"]), _oracle_row(c["ref"][b], seen, c["K"], c["targets"])), (c["name"], b)


# fault -> a case and row of the tables that catches it (every one is caught by many; these are asserted by name)
CAUGHT_BY = {
    "ties_higher_id": ("I3713-nb5-K100-T4", 1, "const"),       # a constant row: the list must be ids 0 .. 99 of the unseen
    "rank_ge": ("I3713-nb5-K100-T4", 1, "const"),              # every item ties with the targets: >= counts the ids behind them too
    "seen_in_rank": ("I6145-nb5-K100-T4", 4, "all_seen"),      # everything seen: every rank is 0
    "neg_zero_below": ("I5121-nb4-K100-T4", 1, "zeros"),       # +0.0 and -0.0 tie: the lower id first, whichever zero it is
    "drop_64q": ("I1025-nb3-K100-T4", 1, "tie64"),             # 9.0 at items 63, 64, 65 and 1023, 1024: items 64 and 1024 are in the list
    "no_padding": ("I8000-nb5-K65-T1", 3, "few_unseen"),       # 64 unseen items, K = 65: slot 64 is -1 / -inf
}


@pytest.mark.parametrize("fault", S.FAULTS)
def test_planted_faults_are_caught(fault):
    """ties broken by the higher id: I3713-nb5-K100-T4 row 1 (const); rank counted with >= in place of >: the same row; seen items
    left in the rank count: I6145-nb5-K100-T4 row 4 (all_seen); -0.0 ordered below +0.0: I5121-nb4-K100-T4 row 1 (zeros); item 64 q
    dropped: I1025-nb3-K100-T4 row 1 (tie64); a list that is not padded: I8000-nb5-K65-T1 row 3 (few_unseen)."""
    name, b, kind = CAUGHT_BY[fault]
    case = next(S.sel_case(*c) for c in S.SEL_CASES if S.sel_case(*c)["name"] == name)
    assert case["kinds"][b] == kind
    _, scores, seen, K, targets = list(S.sel_rows(case))[b]
    ref = S.select_row(scores, seen, K, targets)
    assert S.same_row(ref, _oracle_row(scores, seen, K, targets))
    assert not S.same_row(S.select_row(scores, seen, K, targets, fault=fault), ref), f"{fault} passes {name} row {b}"
    caught = [n for n, s, sn, k, t in _rows() if not S.same_row(S.select_row(s, sn, k, t, fault=fault), S.select_row(s, sn, k, t))]
    print(f"FAULT {fault}: caught by {name} row {b} ({kind}) and {len(caught) - 1} other rows of the tables")
    assert len(caught) >= 1


def test_score_key_orders_what_the_header_says():
    f = lambda *b: np.array(b, dtype=np.uint32).view(np.float32)
    k = S.score_key(f(0xff800000, 0xffc00000, 0xff800001, 0xff7fffff, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x7f7fffff, 0x7f800000,
                      0x7f800001, 0x7fc00000, 0x7fc00001, 0x7fffffff))
    assert k[:3].tolist() == [0, 0, 0]                                   # -inf and the negative NaNs (a signalling one included)
    assert k[3] == 0x00800000 and k[5] == k[6] == 0x80000000             # -FLT_MAX is the first rankable key; -0.0 folds onto +0.0
    assert k[3] < k[4] < k[5] and np.all(np.diff(k[6:10].astype(np.int64)) > 0) and np.all(np.diff(k[11:].astype(np.int64)) > 0)
    assert k[10] == S.score_key(f(0x7fc00001))[0] and k[10] > k[9] and k[11] > k[9]      # a signalling NaN is quieted; NaN above +inf
    finite = np.random.default_rng(3).standard_normal(4096, dtype=np.float32)
    assert np.array_equal(S.key_score(S.score_key(finite)), S.bits(finite))
    assert np.array_equal(np.argsort(S.score_key(finite), kind="stable"), np.argsort(finite, kind="stable"))
    assert S.key_score(S.score_key(f(0x7f800000, 0x7fc00123, 0x7f800001))).tolist() == [0x7f800000, 0x7fc00123, 0x7fc00001]


def test_select_row_on_the_nonfinite_rows():
    """what no oracle states: a positive NaN leads the list (a signalling one quieted), +inf follows, -inf and the negative NaNs are
    in no list; a -inf target ranks behind every rankable item, a NaN target in front of +inf"""
    for n in S.FORM_I:
        c = S.nonfinite_case(n)
        for b in range(c["nb"]):
            seen = c["seen_lists"][b]
            ids, sc, ts, tr = S.select_row(c["scores"][b], seen, c["K"], c["targets"])
            unseen = np.setdiff1d(np.arange(n), seen)
            raw = S.bits(c["scores"][b])
            pos_nan = [i for i in unseen if raw[i] & 0x7fffffff > 0x7f800000 and not raw[i] >> 31]
            excluded = [i for i in unseen if raw[i] >= 0xff800000]
            assert set(ids[:len(pos_nan)].tolist()) == set(pos_nan) and not set(excluded) & set(ids.tolist())
            assert np.all(S.bits(sc[:len(pos_nan)]) & 0x7fc00000 == 0x7fc00000)
            assert np.array_equal(S.bits(ts), raw[c["targets"]])
            n_rankable = len(unseen) - len(excluded)
            for j, t in enumerate(c["targets"]):
                if raw[t] >= 0xff800000:
                    assert tr[j] == n_rankable - (0 if t in seen or t in excluded else 1)
        assert S.select_row(c["scores"][1], c["seen_lists"][1], c["K"], c["targets"])[3][0] < 6      # the NaN target: among the NaNs


def test_bias_order_is_the_oracles_and_no_other():
    c = S.bias_case()
    uid = c["user_ids"]
    ub, ib, mean = c["ub"][uid], c["ib"], np.float32(c["mean"])
    ref = orc.score_rows(c["utab"][uid], c["itab"], ub, ib, c["mean"])
    assert np.array_equal(S.bits(c["ref"]), S.bits(ref))
    dot = orc.score_rows(c["utab"][uid], c["itab"])
    others = {"dot + (ub + ib) + mean": (dot + (ub[:, None] + ib[None, :])) + mean, "(dot + ib) + ub + mean": ((dot + ib[None, :]) + ub[:, None]) + mean,
              "dot + ((ub + ib) + mean)": dot + ((ub[:, None] + ib[None, :]) + mean), "(dot + ub) + (ib + mean)": (dot + ub[:, None]) + (ib[None, :] + mean),
              "(dot + mean) + ub + ib": ((dot + mean) + ub[:, None]) + ib[None, :]}
    for name, alt in others.items():
        differ = np.count_nonzero(S.bits(alt.astype(np.float32)) != S.bits(ref))
        print(f"BIAS {name}: {differ} of {ref.size} scores differ")
        assert differ > 0, name      # (swapping the two biases moves the fewest: both first sums round dot to the same 2^-10 grid)
    for c2 in (S.inst_case(S.PANEL_INSTANTIATIONS[1]), S.edge_case(1921), S.nonfinite_tables_case()):
        uid = c2["user_ids"]
        assert np.array_equal(S.bits(c2["ref"]), S.bits(orc.score_rows(c2["utab"][uid], c2["itab"], c2["ub"][uid], c2["ib"], c2["mean"]))), c2["name"]


def test_nonfinite_tables_give_what_they_are_built_for():
    c, c_inf = S.nonfinite_tables_case(), S.nonfinite_tables_case(with_nan=False)
    ref = S.bits(c["ref"])
    assert np.all(ref[:, S.NONFINITE_ITEMS["nan"]] == 0x7fc00000) and np.isfinite(c_inf["itab"]).all() and np.isfinite(c_inf["utab"]).all()
    keep = np.arange(c["I"]) != S.NONFINITE_ITEMS["nan"]
    assert np.array_equal(ref[:, keep], S.bits(c_inf["ref"])[:, keep]) and np.isfinite(c_inf["ref"][:, S.NONFINITE_ITEMS["nan"]]).all()
    assert np.all(ref[:, S.NONFINITE_ITEMS["pos_inf"]] == 0x7f800000) and np.all(ref[:, S.NONFINITE_ITEMS["neg_inf"]] == 0xff800000)
    others = np.delete(c["ref"], sorted(list(S.NONFINITE_ITEMS.values()) + list(S.NEG_INF_IN_FRONT)), axis=1)
    assert np.isfinite(others).all()
    assert np.all(ref[:, list(S.NEG_INF_IN_FRONT)] == 0xff800000)
    short = c["seen_lists"][int(c["user_ids"][3])]
    special = set(S.NONFINITE_ITEMS.values()) | set(S.NEG_INF_IN_FRONT)
    assert 37 <= c["I"] - len(short) < c["K"] // 2 and not special & set(short.tolist())


def test_header_states_the_panel_paths_requirement():
    """the sentence the strict xfails of tests/test_score_select_forms_gpu.py quote"""
    with open(os.path.join(ROOT, "include", "recad_hip.h")) as f:
        text = " ".join(f.read().replace(" * ", " ").split())
    assert S.HEADER_SAYS in text


# ------------------------------------------------------------------------------------------------------------------ dispatch
def test_dispatch_tables_still_say_what_the_source_says():
    text_of = {}
    for entry in S.SELECT_FORMS + S.SOURCE_FACTS:
        path, line, text = entry[-3:]
        if path not in text_of:
            with open(os.path.join(ROOT, path)) as f:
                text_of[path] = f.read()
        assert text in text_of[path], f"{path} no longer reads `{text}` (it stood near line {line})"
    # the breaks follow from the source's constants: nq = ceil(I / 64) against the NQ ladder, 96 * 64 items, 40 KB of 16-byte-rounded rows
    for lo, hi, form, nq, *_ in S.SELECT_FORMS:
        if form == "wave":
            assert hi == 64 * nq and (lo + 63) // 64 > ([0] + list(S.WAVE_NQ))[S.WAVE_NQ.index(nq)]
    assert S.WAVE_NQ == (16, 32, 48, 58, 64, 80, 88, 96) and S.SELECT_FORMS[8][0] == 96 * 64 + 1
    assert (S.LDS_ROW_MAX_ITEMS * 4 + 15) // 16 * 16 == 40 * 1024 < ((S.LDS_ROW_MAX_ITEMS + 1) * 4 + 15) // 16 * 16
    assert S.SELECT_FORMS[8][1] == S.LDS_ROW_MAX_ITEMS and S.SELECT_FORMS[9][0] == S.LDS_ROW_MAX_ITEMS + 1
    for a, b in zip(S.SELECT_FORMS, S.SELECT_FORMS[1:]):
        assert a[1] + 1 == b[0]


def test_cases_cover_every_instantiation():
    # selection: both ends of every form are in the edge list, and every form is reached by a case
    ends = {x for lo, hi, *_ in S.SELECT_FORMS for x in (lo, hi) if x < 2 ** 31 - 1}
    assert ends == set(S.EDGE_I), sorted(ends ^ set(S.EDGE_I))
    reached = {S.select_form(c[0]) for c in S.SEL_CASES}
    assert reached == {(f[2], f[3]) for f in S.SELECT_FORMS}
    assert [S.select_form(n)[0] for n in S.FORM_I] == ["wave", "lds_rows", "l2_rows"]
    for axis, pos, want in ((2, "K", set(S.K_AXIS)), (3, "T", set(S.T_AXIS))):
        for form in ("wave", "lds_rows", "l2_rows"):
            assert want <= {c[axis] for c in S.SEL_CASES if S.select_form(c[0])[0] == form}, (pos, form)
    assert {c[1] for c in S.SEL_CASES if c[0] in S.EDGE_I} == {1, 3, 4, 5}
    assert max(S.T_AXIS) == S.MAX_TARGETS and S.IN_PASS_TARGETS + 1 in S.T_AXIS and max(S.K_AXIS) == S.MAX_K
    # the candidate counts of the wave kernel's rank loop: constant rows give n_sel = K, rows with K - 1 unseen items n_sel = K - 1
    assert {63, 64, 65, 127, 128, 129} <= set(S.K_AXIS) and "const" in S.ROW_KINDS[5] and "few_unseen" in S.ROW_KINDS[5]
    # panel: 24 instantiations, each the one its case's (nb, I, d, T, request) resolves to; every d and T of the issue's list used
    assert len(set(S.PANEL_INSTANTIATIONS)) == 24
    seen_d, seen_t = set(), set()
    for inst in S.PANEL_INSTANTIATIONS:
        d, T, n, request = S.inst_params(inst)
        assert S.panel_instantiation(S.INST_NB, n, d, T, request) == inst
        assert n % (128 * inst[0]) != 0 and 128 * inst[0] < n < 2 * 128 * inst[0] and S.INST_NB % (16 * inst[3]) != 0
        seen_d.add(d)
        seen_t.add(T)
    assert seen_d == {20, 32, 50, 64, 100, 128, 130, 256} and seen_t == {0, 1, 2, 4}
    # the edge requests: RB 1 and RB 2 above 1024 items, the narrow 16-row form at and below
    assert S.panel_instantiation(33, 1025, 64, 1, S.EDGE_REQUESTS["rows32"]) == (15, 4, 1, 2)
    assert S.panel_instantiation(33, 1025, 64, 1, S.EDGE_REQUESTS["rows16"]) == (15, 4, 1, 1)
    assert S.panel_instantiation(33, 1024, 64, 1, S.EDGE_REQUESTS["rows32"]) == (8, 4, 1, 1)
    # the production choice the issue names: one target, >= 8192 users, dim > 64 -> <15, 8, 1, 2> and <15, 16, 1, 2>
    assert S.panel_instantiation(8192, 34474, 128, 1, {}) == (15, 8, 1, 2) and S.panel_instantiation(8192, 34474, 256, 1, {}) == (15, 16, 1, 2)
    assert (15, 8, 1, 2) in S.PANEL_INSTANTIATIONS and (15, 16, 1, 2) in S.PANEL_INSTANTIATIONS
