"""CPU proof that the budgets of tests/_lightgcn_step_restate.py are usable: on every case of its table a correct fp32 step (the
atomic scatter's sums in shuffled orders, the ordered scatter's in plan order) stays at ratio <= 1 at every stage, and each
planted fault exceeds 1 at the stage it belongs to on at least one element.  The conditions on the inputs (the run of 70, the
17-fold user, the ragged 77, the disjoint rows of steps 0 and 1, N mod 32 != 0, the long row, the marked-block list's condition,
the LDS plan) are asserted here too, from the host builders of the library."""
import ctypes as C

import numpy as np
import pytest

from recad_amd import _lib

from . import _lightgcn_step_restate as S
from ._lds_restate import build_plan


@pytest.fixture(scope="module")
def world():
    """graphs, operators and triplets: built once, shared, never modified"""
    memo = {}

    def get(which, path):
        if which not in memo:
            g = S.graph(which)
            rowptr, col = S.adjacency(g)
            memo[which] = {"g": g, "rowptr": rowptr, "col": col, "val": S.host_val(rowptr, col), "trip": S.triplets(g)}
        w = memo[which]
        if path not in w:
            w[path] = S.Operator(w["rowptr"], w["col"], w["val"], path, w["g"]["U"])
        return w, w[path]
    return get


def _schedule(rowptr, n_users, dim):
    """(plain blocks, scratch words) of the row-gather schedule"""
    h, nb, nw, sw = C.c_void_p(), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    _lib.check(_lib.lib().rk_csr_schedule_build_host(len(rp) - 1, rp.ctypes.data_as(C.c_void_p), n_users, dim, C.byref(h), C.byref(nb), C.byref(nw),
                                                     C.byref(sw)), "rk_csr_schedule_build_host")
    _lib.lib().rk_csr_schedule_destroy(h)
    return nb.value & 0x07ffffff, int(sw.value)


def test_inputs_reach_every_branch(world):
    w, _ = world(1, "rg")
    g, (users, pos, neg) = w["g"], w["trip"]
    U, N = g["U"], g["N"]
    assert N % 32 != 0 and len(users) == S.N_TRIP == 3 * S.BATCH - 19
    assert S.window(w["trip"], 2)[1] == 77
    deg_u, deg_i = np.diff(g["r_ptr"]), np.bincount(g["r_idx"], minlength=g["I"])
    assert deg_u[S.ISO_USER] == 0 and (deg_u == 0).sum() == 1 and deg_i[S.ISO_ITEM] == 0 and deg_i[S.HUB_ITEM] == U - 1
    for dim in (64, 100, 256):
        assert ((deg_u > 0) & (deg_u <= dim // 4)).any() and (deg_u > dim // 4).any()
        blocks, scratch = _schedule(w["rowptr"], U, dim)
        assert scratch > 0, "no long row: the scratch hand-off is not exercised"
        words, info = build_plan(U, g["I"], w["rowptr"], w["col"], w["val"], dim)
        assert words is not None and info.n_wg > 0, "the graph does not qualify for the LDS plan"
    (u0, p0, n0), _ = S.window(w["trip"], 0)
    assert (p0 == S.DUAL_ITEM).sum() == S.RUN[0] and (n0 == S.DUAL_ITEM).sum() == S.RUN[1] and sum(S.RUN) == 70
    assert (u0 == S.USER17).sum() == 17 and (n0 == S.ISO_ITEM).any() and not (users == S.ISO_USER).any()
    rows0 = np.unique(np.concatenate(S.node_rows(g, (u0, p0, n0))))
    rows1 = np.unique(np.concatenate(S.node_rows(g, S.window(w["trip"], 1)[0])))
    assert len(np.intersect1d(rows0, rows1)) == 0
    assert not np.any(pos == neg)
    # the second graph: the condition of launch_forward for the marked-block list at L = 3
    w2, _ = world(2, "rg")
    blocks, scratch = _schedule(w2["rowptr"], w2["g"]["U"], 64)
    assert scratch > 0 and 2 * (3 * S.BATCH + scratch // 64 + 1) <= blocks, (blocks, scratch)
    blocks1, scratch1 = _schedule(w["rowptr"], U, 64)
    assert 2 * (3 * S.BATCH + scratch1 // 64 + 1) > blocks1, "the first graph would do: the second is not needed"


_WALKS = {}


def _walk(world, case, step, ordered):
    """the float64 walk of a step of a case: computed once, shared, never modified"""
    variant, d, L, lam, t0 = case
    closed = S.counted(variant, ordered)
    key = (case, step, closed)
    if key not in _WALKS:
        w, op = world(S.graph_of(variant), S.path_of(variant))
        win, nb = S.window(w["trip"], step)
        rows = S.node_rows(w["g"], win)
        E0, m, v = S.state(w["g"], d, seed=100 * d + L)
        ref = S.step64(op, E0, L, lam, rows, nb, closed)
        adam = S.adam64(E0, ref["grad"], ref["b_grad"], m, v, t0 + step + 1)
        _WALKS[key] = (op, (E0, m, v), rows, nb, closed, ref, adam)
    return _WALKS[key]


def _ratios(ref, adam, got):
    r = {"light": S.ratio_mutant(got["light"], ref["light"], ref["b_light"]), "loss": abs(got["loss"] - ref["loss"]) / ref["b_loss"],
         "grad": S.ratio_mutant(got["grad"], ref["grad"], ref["b_grad"])}
    for k, name in enumerate("pmv"):
        r[name] = S.ratio_mutant(got["adam"][k], adam[0][k], adam[1][k])
    return r


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_correct_fp32_step_stays_inside(world, case):
    variant, d, L, lam, t0 = case
    for step in (0, 1, 2):
        for ordered in (False, True):
            op, (E0, m, v), rows, nb, closed, ref, adam = _walk(world, case, step, ordered)
            seeds = (1, 2, 3) if S.graph_of(variant) == 1 else (1 + step,)      # (the large graph: one order per step, three in all)
            for rng in ([None] if ordered else [np.random.default_rng(s) for s in seeds]):
                got = S.step32(op, E0, m, v, L, lam, rows, nb, t0 + step + 1, closed, rng=rng)
                r = _ratios(ref, adam, got)
                print(f"RATIO host {S.case_id(case)} step {step} {'ordered' if ordered else 'atomic'} " + " ".join(f"{k} {x:.4f}" for k, x in r.items()))
                assert max(r.values()) <= 1.0, r
            # the isolated user: propagation leaves fl(E0 / (L + 1)), the gradient is an exact zero
            iso = S.ISO_USER if S.graph_of(variant) == 1 else None
            if iso is not None:
                assert np.all(ref["b_grad"][iso] == 0) and np.all(ref["grad"][iso] == 0)


# the stage at which each planted fault must show, and the step it is planted in
FAULTS = {"drop_incidence": ("grad", 0), "reg_once_fewer": ("grad", 0), "ragged_invb": ("grad+loss", 2), "inv_layers": ("light", 0),
          "frontier_drop": ("grad", 0), "residue": ("grad", 1), "swap_mv": ("pmv", 0)}


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_planted_faults_fall_outside(world, case):
    variant, d, L, lam, t0 = case
    assert set(FAULTS) == set(S.MUTANTS)
    for ordered in (False, True):
        for mutant, (stage, step) in FAULTS.items():
            if (mutant == "reg_once_fewer" and lam == 0) or (mutant in ("inv_layers", "frontier_drop") and L == 0):
                continue        # the fault does not exist there: no regulariser, no layer
            op, (E0, m, v), rows, nb, closed, ref, adam = _walk(world, case, step, ordered)
            residue = None
            if mutant == "residue":      # one row of step 0's gprop that step 1 does not touch
                _, _, rows0, nb0, _, _, _ = _walk(world, case, 0, ordered)
                g0 = S.step32(op, E0, m, v, L, lam, rows0, nb0, t0 + 1, closed)["gprop"]
                residue = np.zeros_like(g0)
                r0 = rows0[1][0]
                assert r0 not in np.concatenate(rows) and np.any(g0[r0] != 0)
                residue[r0] = g0[r0]
            got = S.step32(op, E0, m, v, L, lam, rows, nb, t0 + step + 1, closed, rng=None if ordered else np.random.default_rng(4), mutant=mutant,
                           residue=residue)
            r = _ratios(ref, adam, got)
            print(f"RATIO host-fault {mutant} {S.case_id(case)} {'ordered' if ordered else 'atomic'} " + " ".join(f"{k} {x:.3g}" for k, x in r.items()))
            for s in {"grad": ["grad"], "light": ["light"], "grad+loss": ["grad", "loss"], "pmv": ["p", "m", "v"]}[stage]:
                assert r[s] > 1.0, (mutant, s, r)
