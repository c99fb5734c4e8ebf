"""GPU tests of csrc/uba.hip, one entry point at a time against the float64 restatement (tests/_uba_restate.py): rk_uba_redraw in
its replay form and with its own draws, rk_uba_scores in both modes and on both paths, rk_uba_prob on the reference's recorded
draws (tests/golden/uba_prob_elementwise.npz) and in the matrix mode, rk_uba_workspace_bytes and every refusal.

Bounds.  None: ratings are integers 1..5, every product and sum is an integer below 2^53 (the entry points refuse shapes where
it might not be), the kernels add in int64 and the restatement in float64, so every comparison is an equality.

Shapes.  n_items 63 / 64 / 65 around the wave size and 257 (more than one pass of every 64- and 256-wide loop, with one row of
200 ratings); n_users = the target users plus one, 96, 300; 1, 3 and 50 target users; budget steps 1 and 6; the selected item at
0, in the middle and at n_items - 1.  Crafted rows: target user 0 rated nothing, target users 1 and 2 share their items (so
redrawn rows meet in the weights), item 2 is rated by nobody, the selected item is rated by some target users and not by
others.  Both paths of the one shape switch (weights in LDS / in the scratch) are forced at every shape, and AUTO is checked
against them."""
import ctypes as C

import numpy as np
import pytest
import torch

from recad_amd import _lib
from recad_amd.attack.uba import rating_csc

from . import _golden as G
from . import _uba_restate as R

pytestmark = pytest.mark.gpu
EINVAL = -22
ITEMS = (63, 64, 65, 257)
USERS = ("targets+1", 96, 300)
TARGETS = (1, 3, 50)
MODES = {"elementwise": _lib.RK_UBA_ELEMENTWISE, "matrix": _lib.RK_UBA_MATRIX}
PATHS = (_lib.RK_UBA_PATH_LDS, _lib.RK_UBA_PATH_WORK, _lib.RK_UBA_PATH_AUTO)


def _t(a, dtype, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _hptr(a):
    return a.ctypes.data_as(C.c_void_p)


def craft(I, U, n_t, seed):
    """(mat [U, I] float64, targets): see the module docstring."""
    U = n_t + 1 if U == "targets+1" else U
    rng = np.random.default_rng(seed)
    mat = np.zeros((U, I))
    for u in range(U):
        n = int(rng.integers(1, 24))
        mat[u, rng.choice(I, size=n, replace=False)] = rng.integers(1, 6, size=n)
    targets = rng.choice(U, size=n_t, replace=False)
    mat[targets[0]] = 0                                     # an empty row before the redraw
    if n_t >= 3:
        mat[targets[2]] = mat[targets[1]]                   # two target users who share every item
    if I == 257:
        u = targets[-1]
        mat[u] = 0
        mat[u, rng.choice(I, size=200, replace=False)] = rng.integers(1, 6, size=200)
    mat[:, 2] = 0                                           # an item nobody rated
    return mat, targets.astype(np.int32)


class Data:
    def __init__(self, dev, mat, targets):
        self.dev, self.mat, self.targets = dev, mat, np.ascontiguousarray(targets, dtype=np.int32)
        self.U, self.I = mat.shape
        nz = mat != 0
        ptr = np.zeros(self.U + 1, dtype=np.int64)
        ptr[1:] = np.cumsum(nz.sum(axis=1))
        idx, val = np.nonzero(nz)[1].astype(np.int32), mat[nz].astype(np.float32)
        self.nnz = len(idx)
        colptr, crow, cval = rating_csc(self.U, self.I, ptr, idx, val)
        self.rowptr, self.col = _t(ptr, np.int32, dev), _t(np.append(idx, 0), np.int32, dev)
        self.colptr, self.crow, self.cval = _t(colptr, np.int32, dev), _t(np.append(crow, 0), np.int32, dev), _t(np.append(cval, 0), np.float32, dev)

    def side(self, s):
        ptr, col = R.side_layout(self.mat, self.targets, s)
        return ptr, col, int(ptr[-1])

    def redraw(self, s, b, trial, draws, seed=7, cap=None, targets=None, **over):
        targets = self.targets if targets is None else np.ascontiguousarray(targets, dtype=np.int32)
        n = len(targets)
        cap = self.side(s)[2] if cap is None else cap
        out = {"ptr": torch.full((max(n, 1) + 1,), -7, dtype=torch.int32, device=self.dev),
               "col": torch.full((max(cap, 1),), -7, dtype=torch.int32, device=self.dev),
               "val": torch.full((max(cap, 1),), -7, dtype=torch.int32, device=self.dev),
               "status": torch.zeros(1, dtype=torch.int32, device=self.dev)}
        d = None if draws is None else _t(draws, np.int32, self.dev)
        a = dict(n_users=self.U, n_items=self.I, n_targets=n, s=s, b=b, trial=trial, cap=cap)
        a.update(over.pop("over", {}), **over)
        rc = _lib.lib().rk_uba_redraw(a["n_users"], a["n_items"], self.nnz, _lib.ptr(self.rowptr), _lib.ptr(self.col), _hptr(targets), a["n_targets"],
                                      a["s"], a["b"], a["trial"], _lib.ptr(d), seed, a["cap"], _lib.ptr(out["ptr"]), _lib.ptr(out["col"]),
                                      _lib.ptr(out["val"]), _lib.ptr(out["status"]), _lib.stream_ptr(self.dev))
        return rc, {k: v.cpu().numpy() for k, v in out.items()}

    def scores(self, side_ptr, side_col, side_val, s, b, mode, path, want_x=True, targets=None, **over):
        targets = self.targets if targets is None else np.ascontiguousarray(targets, dtype=np.int32)
        n, cap = len(targets), len(side_col)
        counts = torch.full((3 * max(n, 1),), -7, dtype=torch.int32, device=self.dev)
        x = torch.full((max(n, 1) * self.I,), -7.0, dtype=torch.float64, device=self.dev) if want_x else None
        sp, sc, sv = _t(side_ptr, np.int32, self.dev), _t(side_col, np.int32, self.dev), _t(side_val, np.int32, self.dev)
        a = dict(n_users=self.U, n_items=self.I, n_targets=n, s=s, b=b, mode=mode, path=path, cap=cap)
        a.update(over.pop("over", {}), **over)
        rc = _lib.lib().rk_uba_scores(a["n_users"], a["n_items"], self.nnz, _lib.ptr(self.colptr), _lib.ptr(self.crow), _lib.ptr(self.cval),
                                      _hptr(targets), a["n_targets"], _lib.ptr(sp), _lib.ptr(sc), _lib.ptr(sv), a["cap"], a["s"], a["b"], a["mode"],
                                      a["path"], _lib.ptr(counts), _lib.ptr(x), _lib.stream_ptr(self.dev))
        return rc, counts.cpu().numpy().reshape(3, -1), None if x is None else x.cpu().numpy().reshape(-1, self.I)

    def prob(self, s, budget, mode, path, draws, seed=7, cap=None, targets=None):
        targets = self.targets if targets is None else np.ascontiguousarray(targets, dtype=np.int32)
        n = len(targets)
        cap = self.side(s)[2] if cap is None else cap
        prob = np.full((max(n, 1), max(budget, 1)), -7.0)
        ties = C.c_int32(-7)
        d = None if draws is None else _t(draws, np.int32, self.dev)
        rc = _lib.lib().rk_uba_prob(self.U, self.I, self.nnz, _lib.ptr(self.rowptr), _lib.ptr(self.col), _lib.ptr(self.colptr), _lib.ptr(self.crow),
                                    _lib.ptr(self.cval), _hptr(targets), n, s, budget, mode, path, _lib.ptr(d), seed, cap, _hptr(prob),
                                    C.byref(ties), _lib.stream_ptr(self.dev))
        return rc, prob, int(ties.value)


def positions(I):
    return (0, I // 2, I - 1)


# ---------------------------------------------------------------- rk_uba_redraw
@pytest.mark.parametrize("n_t", TARGETS)
@pytest.mark.parametrize("U", USERS)
@pytest.mark.parametrize("I", ITEMS)
def test_redraw(gpu_device, I, U, n_t):
    mat, targets = craft(I, U, n_t, seed=1000 * I + n_t)
    d = Data(gpu_device, mat, targets)
    rng = np.random.default_rng(I + n_t)
    rated = 0
    for s in positions(I):
        mat[targets[n_t // 2], s] = 4                        # rated by one target user; the others get it inserted
        d = Data(gpu_device, mat, targets)
        ptr, col, cap = d.side(s)
        rated += int((mat[targets, s] != 0).sum())
        draws = rng.integers(1, 6, size=cap)
        rc, out = d.redraw(s, 1, 0, draws)
        _lib.check(rc, "rk_uba_redraw")
        _, val = R.redraw(mat, targets, s, draws)
        assert out["status"][0] == 0 and np.array_equal(out["ptr"], ptr) and np.array_equal(out["col"], col) and np.array_equal(out["val"], val)
        # its own draws: the same layout, 1..5 everywhere, 5 at s, the same for the same key, another stream for another key
        own = [d.redraw(s, b, trial, None, seed=seed)[1] for b, trial, seed in ((6, 3, 7), (6, 3, 7), (6, 4, 7), (1, 3, 7), (6, 3, 8))]
        for o in own:
            assert np.array_equal(o["ptr"], ptr) and np.array_equal(o["col"], col) and o["val"].min() >= 1 and o["val"].max() <= 5
            assert (o["val"][col == s] == 5).all()
        assert np.array_equal(own[0]["val"], own[1]["val"])
        if cap > 40:                                         # 5^-40: long enough that two streams cannot agree by chance
            assert all(not np.array_equal(own[0]["val"], o["val"]) for o in own[2:])
    assert rated >= 1
    assert np.array_equal(d.rowptr.cpu().numpy()[1:], np.cumsum((mat != 0).sum(axis=1)))       # the rating CSR is only read


def test_redraw_values_are_uniform(gpu_device):
    mat, targets = craft(257, 96, 50, seed=3)
    d = Data(gpu_device, mat, targets)
    vals = np.concatenate([d.redraw(5, 2, trial, None, seed=11)[1]["val"] for trial in range(10)])
    n = len(vals)
    assert n > 5000
    # each value has probability 1/5 (up to the 5 fixed at s): six standard deviations of a binomial count
    freq = np.bincount(vals, minlength=6)[1:]
    assert np.all(np.abs(freq - n / 5) <= 6 * np.sqrt(n * 0.16) + 10 * 50), freq


# ---------------------------------------------------------------- rk_uba_scores
@pytest.mark.parametrize("n_t", TARGETS)
@pytest.mark.parametrize("U", USERS)
@pytest.mark.parametrize("I", ITEMS)
def test_scores(gpu_device, I, U, n_t):
    mat, targets = craft(I, U, n_t, seed=2000 * I + n_t)
    rng = np.random.default_rng(I * 7 + n_t)
    for k, s in enumerate(positions(I)):
        mat[targets[n_t // 2], s] = 3
        d = Data(gpu_device, mat, targets)
        ptr, col, cap = d.side(s)
        draws = rng.integers(1, 6, size=cap)
        if k == 1:
            draws[:] = 5                                     # every redrawn rating equal: ties on both sides of s
        red, val = R.redraw(mat, targets, s, draws)
        for b in (1, 6):
            ref = {"elementwise": R.scores_elementwise(red, targets), "matrix": R.scores_matrix_weighted(red, targets, b)}
            if U != 300 and b == 1:
                assert np.array_equal(ref["matrix"], R.scores_matrix_literal(red, targets, b))
            for mode, code in MODES.items():
                for path in PATHS:
                    rc, counts, x = d.scores(ptr, col, val, s, b, code, path)
                    _lib.check(rc, "rk_uba_scores")
                    assert np.array_equal(x, ref[mode]), (s, b, mode, path, np.abs(x - ref[mode]).max())
                    assert np.array_equal(counts, np.stack(R.counts(ref[mode], s))), (s, b, mode, path)
                    assert (x[:, 2] == 0).all()
        rc, counts, x = d.scores(ptr, col, val, s, 6, MODES["matrix"], _lib.RK_UBA_PATH_AUTO, want_x=False)    # x is optional
        _lib.check(rc, "rk_uba_scores")
        assert x is None and np.array_equal(counts, np.stack(R.counts(ref["matrix"], s)))


# ---------------------------------------------------------------- rk_uba_prob
@pytest.fixture(scope="module")
def prob_golden():
    g = G.load("uba_prob_elementwise")
    mat = g["train_mat"].astype(np.float64)
    targets, s, budget = g["target_user_ids"].astype(np.int32), int(g["selected_id"]), int(g["budget"])
    ref = {mode: R.prob(mat, targets, s, budget, g["draws"], mode) for mode in MODES}
    return g, mat, targets, s, budget, ref


def test_prob_on_the_reference_draws(gpu_device, prob_golden):
    g, mat, targets, s, budget, ref = prob_golden
    d = Data(gpu_device, mat, targets)
    prob_ref, n_tie, hits, ties = ref["elementwise"]
    rc, prob, dev_ties = d.prob(s, budget, MODES["elementwise"], _lib.RK_UBA_PATH_AUTO, g["draws"])
    _lib.check(rc, "rk_uba_prob")
    print("tie-dependent", dev_ties, "of", ties.size)
    assert dev_ties == n_tie and 0 < n_tie / ties.size <= 0.10
    assert np.array_equal(prob, prob_ref)
    # against the reference's own hits: every (target user, budget step) without a tie-dependent trial agrees exactly, the
    # others differ by at most their number of tie-dependent trials
    ref_hits = g["positions"] != 0
    assert np.array_equal(ref_hits[~ties], hits[~ties])
    quiet = ~ties.any(axis=1).T
    assert np.array_equal(prob[quiet], g["prob_mat"][quiet])
    assert np.all(np.abs(prob - g["prob_mat"]) * R.TRIALS <= ties.sum(axis=1).T + 1e-9)
    assert np.array_equal(d.rowptr.cpu().numpy()[1:], np.cumsum((mat != 0).sum(axis=1)))


@pytest.mark.parametrize("path", PATHS)
def test_prob_matrix_mode(gpu_device, prob_golden, path):
    g, mat, targets, s, budget, ref = prob_golden
    d = Data(gpu_device, mat, targets)
    prob_ref, n_tie, hits, _ = ref["matrix"]
    rc, prob, dev_ties = d.prob(s, budget, MODES["matrix"], path, g["draws"])
    _lib.check(rc, "rk_uba_prob")
    assert np.array_equal(prob, prob_ref) and dev_ties == n_tie


def test_prob_own_draws_budget_one_and_repeatable(gpu_device):
    mat, targets = craft(65, 96, 3, seed=5)
    d = Data(gpu_device, mat, targets)
    a = d.prob(64, 1, MODES["matrix"], _lib.RK_UBA_PATH_AUTO, None, seed=5)
    b = d.prob(64, 1, MODES["matrix"], _lib.RK_UBA_PATH_WORK, None, seed=5)
    _lib.check(a[0], "rk_uba_prob")
    assert a[1].shape == (3, 1) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.all((a[1] >= 0) & (a[1] <= 1)) and np.array_equal(a[1] * 10, np.round(a[1] * 10))


# ---------------------------------------------------------------- rk_uba_workspace_bytes and the refusals
def test_workspace_bytes():
    nb = C.c_int64(-1)
    L = _lib.lib()
    assert L.rk_uba_workspace_bytes(6040, 3706, 50, 9000, 6, C.byref(nb)) == 0
    assert nb.value >= 50 * 6040 * 8 + 50 * 3706 * 8 + 2 * 9000 * 4 and nb.value < 8 << 20
    for bad in ((0, 64, 3, 10, 6), (96, 0, 3, 10, 6), (96, 64, 0, 10, 6), (96, 64, 65, 100, 6), (96, 64, 3, 2, 6), (96, 64, 3, 3 * 64 + 1, 6),
                (96, 64, 3, 10, 0), (96, 64, 3, 10, _lib.RK_UBA_MAX_BUDGET + 1)):
        nb = C.c_int64(-1)
        assert L.rk_uba_workspace_bytes(*bad, C.byref(nb)) == EINVAL and nb.value == -1, bad
    assert L.rk_uba_workspace_bytes(96, 64, 3, 10, 6, None) == EINVAL


def test_refusals_return_their_status_without_launching(gpu_device):
    mat, targets = craft(64, 96, 3, seed=9)
    d = Data(gpu_device, mat, targets)
    s = 5
    ptr, col, cap = d.side(s)
    _, val = R.redraw(mat, targets, s, np.ones(cap, dtype=np.int64))
    big = _lib.RK_UBA_LDS_USERS + 1
    bad_targets = ([], list(range(65)), [1, 2, 1], [96, 1, 2], [-1, 1, 2])
    for tg in bad_targets:
        rc, out = d.redraw(s, 1, 0, None, targets=np.asarray(tg, dtype=np.int32), cap=cap)
        assert rc == EINVAL and all((v == -7).all() for k, v in out.items() if k != "status") and out["status"][0] == 0, tg
        rc, counts, x = d.scores(ptr, col, val, s, 1, 0, 0, targets=np.asarray(tg, dtype=np.int32))
        assert rc == EINVAL and (counts == -7).all() and (x == -7).all(), tg
        rc, prob, ties = d.prob(s, 6, 0, 0, None, targets=np.asarray(tg, dtype=np.int32), cap=cap)
        assert rc == EINVAL and (prob == -7).all() and ties == -7, tg
    for over in (dict(s=-1), dict(s=64), dict(b=0), dict(b=_lib.RK_UBA_MAX_BUDGET + 1), dict(cap=2), dict(cap=3 * 64 + 1), dict(n_users=0),
                 dict(n_items=0), dict(trial=-1)):
        rc, out = d.redraw(s, 1, 0, None, over=over)
        assert rc == EINVAL and all((v == -7).all() for k, v in out.items() if k != "status"), over
    for over in (dict(s=-1), dict(s=64), dict(b=0), dict(b=_lib.RK_UBA_MAX_BUDGET + 1), dict(mode=2), dict(mode=-1), dict(path=3), dict(path=-1),
                 dict(n_users=big, path=_lib.RK_UBA_PATH_LDS, mode=1), dict(n_users=0), dict(n_items=0), dict(cap=2)):
        rc, counts, x = d.scores(ptr, col, val, s, 1, 0, 0, over=over)
        assert rc == EINVAL and (counts == -7).all() and (x == -7).all(), over
        assert _lib.lib().rk_last_error()
    for kw in (dict(budget=0), dict(budget=_lib.RK_UBA_MAX_BUDGET + 1), dict(mode=2), dict(path=3), dict(s=64)):
        a = dict(s=s, budget=6, mode=0, path=0)
        a.update(kw)
        rc, prob, ties = d.prob(a["s"], a["budget"], a["mode"], a["path"], None)
        assert rc == EINVAL and (prob == -7).all() and ties == -7, kw
    # rows that do not fit side_cap: the redraw writes nothing and says so; rk_uba_prob turns that into its status
    rc, out = d.redraw(s, 1, 0, None, cap=cap - 1)
    assert rc == 0 and out["status"][0] == 1 and all((v == -7).all() for k, v in out.items() if k != "status")
    rc, prob, ties = d.prob(s, 2, 1, 0, None, cap=cap - 1)
    assert rc == EINVAL and (prob == -7).all()
    # a shape whose three-hop scores could leave the exact range is refused in the matrix mode only (nothing is launched:
    # the arrays are those of the small shape)
    rc, counts, x = d.scores(ptr, col, val, s, 1, 1, _lib.RK_UBA_PATH_WORK, n_users=1 << 30, n_items=1 << 30, cap=3)
    assert rc == EINVAL and (counts == -7).all()
