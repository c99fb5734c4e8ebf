"""CPU checks of the LDS-resident SpMM's plan (recad_amd/csrc/spmm_lds.hip): rk_lds_plan_build_host is pure host code, so
the schedule can be validated without a GPU -- a numpy walk of the plan in exactly the order the kernel consumes it
(tasks -> chunk partials -> per-row sums -> dinv scaling) must reproduce the normalised adjacency product, every stored
entry must appear exactly once in the column stream, and graphs that do not qualify must be refused."""
import numpy as np
import pytest

from recad_amd import synth

from tests._lds_restate import H, LB, build_plan, check_multi_queues, emulate, norm_adj_csr  # noqa: F401  (test_host_sanitizers.py and test_gpu_parity.py import norm_adj_csr from here)


@pytest.mark.parametrize("shape,dim", [("tiny", 64), ("tiny", 32), ("tiny", 128)])
def test_plan_reproduces_the_product(shape, dim):
    data = synth.make(shape)
    U, I = data["n_users"], data["n_items"]
    rowptr, col, val = norm_adj_csr(U, I, *data["train"])
    words, info = build_plan(U, I, rowptr, col, val, dim, n_cu=64)
    assert words is not None and int(words[H["MAGIC"]]) == 0x4c445331
    assert info.n_wg == int(words[H["NWG"]]) and info.lds_bytes <= 160 * 1024 - 64
    rng = np.random.default_rng(5)
    x = rng.standard_normal((U + I, dim)).astype(np.float32)
    y, entries = emulate(words, x)
    assert entries == len(col)        # every stored entry exactly once (per slice)
    ref = np.zeros((U + I, dim), dtype=np.float64)
    rows = np.repeat(np.arange(U + I), np.diff(rowptr))
    np.add.at(ref, rows, val.astype(np.float64)[:, None] * x[col].astype(np.float64))
    assert np.abs(y - ref).max() <= 2e-6 * np.abs(ref).max()


def test_plan_ml1m_shape_fits_and_balances():
    data = synth.make("ml1m")
    U, I = data["n_users"], data["n_items"]
    rowptr, col, val = norm_adj_csr(U, I, *data["train"])
    words, info = build_plan(U, I, rowptr, col, val, 64, n_cu=256)
    assert words is not None
    assert info.n_wg == 256 and (info.lpa, info.lpb) == (1, 1)     # 4-float slices of both tables: one lane per entry
    # per-block work (stream units) within 15 % of the mean in each half
    nb0, nb1 = int(words[H["NBLK0"]]), int(words[H["NBLK1"]])
    for lo, hi in ((0, nb0), (nb0, nb0 + nb1)):
        units = []
        for bi in range(lo, hi):
            bd = words[int(words[H["BLK_OFS"]]) + bi * LB["WORDS"]:][: LB["WORDS"]]
            t = words[int(bd[LB["TASK_OFS"]]): int(bd[LB["TASK_OFS"]]) + 2 * int(bd[LB["NTASKS"]])].reshape(-1, 2)
            units.append(int(t[:, 1].sum()))
        units = np.asarray(units, dtype=np.float64)
        assert units.max() <= 1.15 * units.mean(), units


def test_plan_refuses_graphs_that_do_not_qualify():
    data = synth.make("tiny")
    U, I = data["n_users"], data["n_items"]
    rowptr, col, val = norm_adj_csr(U, I, *data["train"])
    bad = val.copy()
    bad[7] *= 1.01                       # not dinv[r]*dinv[c] any more
    assert build_plan(U, I, rowptr, col, bad, 64)[0] is None
    col2 = col.copy()
    col2[0] = 0                          # a user row pointing at a user column: not bipartite
    assert build_plan(U, I, rowptr, col2, val, 64)[0] is None
    assert build_plan(U, I, rowptr, col, val, 6)[0] is None      # dim % 4
    # a class table that cannot fit 160 KB of LDS at the narrowest slice
    Ub, Ib = 70000, 200
    ptr = np.arange(Ub + 1, dtype=np.int64)
    idx = (np.arange(Ub) % Ib).astype(np.int32)
    rp, cc, vv = norm_adj_csr(Ub, Ib, ptr, idx)
    assert build_plan(Ub, Ib, rp, cc, vv, 64)[0] is None


@pytest.mark.parametrize("shape,dim,n_cu", [("tiny", 64, 64), ("tiny", 32, 64), ("tiny", 16, 64), ("tiny", 128, 256), ("tiny", 256, 256), ("ml1m", 64, 256)])
def test_multi_phase_queues_cover_the_launch_and_cannot_deadlock(shape, dim, n_cu):
    """spmm_lds_multi_kernel's contract with the plan: the queue lists hold every (half, slice, block) workgroup of the
    single-phase table exactly once; a column group (the workgroups that exchange data between consecutive layers) never
    straddles queues and its member count is what the arrival counter waits for; and -- simulated with FEWER resident
    workgroups than the grid, in adversarial order -- handing a queue's items out in phase-major ticket order never leaves a
    running workgroup waiting for an item nobody has taken."""
    data = synth.make(shape)
    U, I = data["n_users"], data["n_items"]
    rowptr, col, val = norm_adj_csr(U, I, *data["train"])
    words, info = build_plan(U, I, rowptr, col, val, dim, n_cu=n_cu)
    assert words is not None
    check_multi_queues(words, dim)     # (tests/_lds_restate.py: the forced forms of test_spmm_lds_forms_host.py take the same checks)


def test_plan_builder_leaves_the_callers_affinity_alone():
    """The builder places its pool's short-lived workers on CPUs of the caller's mask (host/lds_plan_host.h: place_self).  A first
    version set the workers' affinity from OUTSIDE: a worker that had already finished has thread id 0, and the call then pinned
    the CALLER -- every later thread and child process of the host program inherited one CPU.  Tiny graphs (more threads than
    work: workers exit at once) are the case that showed it."""
    import os
    if not hasattr(os, "sched_getaffinity"):
        pytest.skip("no sched_getaffinity on this platform")
    before = os.sched_getaffinity(0)
    rng = np.random.default_rng(7)
    for k in range(40):
        U, I = int(rng.integers(20, 400)), int(rng.integers(20, 400))
        deg = rng.integers(1, min(I, 12), U)
        ptr = np.zeros(U + 1, dtype=np.int64)
        ptr[1:] = np.cumsum(deg)
        idx = np.concatenate([np.sort(rng.choice(I, size=int(n), replace=False)) for n in deg])
        words, _ = build_plan(U, I, *norm_adj_csr(U, I, ptr, idx), 64)
        assert words is not None
        assert os.sched_getaffinity(0) == before, k
