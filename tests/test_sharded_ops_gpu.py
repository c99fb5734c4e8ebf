"""GPU tests of the op-level C ABI the row-sharded and 2-D trainers build a step from, one entry point at a time against the
float64 restatement and its error budgets (tests/_sharded_ops_restate.py; tests/test_sharded_ops_host.py shows that a correct
fp32 implementation stays inside them and that a dropped incidence or a swapped sign does not): rk_bpr_rows_ordered, rk_bpr_rows,
rk_rows_gather_masked, rk_rows_zero, rk_rows_mark_bits, rk_spmm_csr_ex and rk_adam_coef_advance with rk_adam_step / _dev.

Every floating-point comparison is per element against that element's own budget; everything else is an equality of bits.
Each test prints its worst |got - ref| / bound ("RATIO <entry point> <value>") before it asserts.

Shapes are the smallest at which each branch of the kernels can still go wrong, not the workload's.  BPR: runs of 1, 15, 16, 17,
63, 64, 65, 128, 129, 200 incidences and one of 67 with mixed roles (the 16-incidence coefficient rounds and the 64-incidence
chunks of bpr_rows_kernel), d = 64 / 128 / 256 (Q = 1, 2, 4 on the vec4 path) and 7 / 50 / 100 / 130 (the scalar path; 130 is
Q = 4 with a tail, 7 fewer lanes than a group stride), batches of 1, 5, 1061 and 1400 triplets (4200 incidences > 256 * 16: the
second trip of the plan loop), L = 0 and 3, lambda = 0, 1e-4 and 0.5.  Whether the trainers' own batches hold a run longer than
16 or 64 incidences was not measured; the runs are covered here instead.  SpMM: ~600 rows with empty rows, rows on both sides
of dim / 4 nonzeros (the packed and the segment path), one row of every column (the long-row scratch hand-off), square and
with x twice as tall; d = 32 / 64 / 128 / 256 (vector kernel) and 48 / 100 (generic kernel).  Index kernels: the grid-stride
trips (n > 16384 rows, n > 262144 bits), duplicates, guard bands."""
import ctypes as C

import numpy as np
import pytest
import torch

from recad_amd import _lib
from recad_amd.sharded import HipOps

from . import _sharded_ops_restate as R

pytestmark = pytest.mark.gpu
EINVAL = -22
SENT_BITS = np.float32(R.SENTINEL).view(np.uint32)
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def _t(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ratio(got, ref, bound):
    """worst |got - ref| / bound; an element whose budget is zero must be exact"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert np.all(np.isfinite(err)), "non-finite output"
    assert np.all(err[bound == 0] == 0)
    return float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)))


def _report(entry, value):
    print(f"RATIO {entry} {value:.4f}")


# ================================================================ BPR
@pytest.fixture(scope="module")
def bpr_ref():
    """case, float64 restatement and budgets of one (nb, d, L, lam): computed once, shared, never modified"""
    cases, refs = {}, {}

    def get(nb, d, L, lam):
        if (nb, d) not in cases:
            cases[nb, d] = R.bpr_case(nb, d, seed=1000 * nb + d)
        c = cases[nb, d]
        if (nb, d, L, lam) not in refs:
            ref = R.bpr(d, L, lam, c["light"], c["emb"], c["ru"], c["rp"], c["rn"])
            refs[nb, d, L, lam] = (ref, R.bpr_bounds(ref, d, lam, c["emb"], nb))
        return (c,) + refs[nb, d, L, lam]
    return get


class BprRun:
    """device copies of a case; every call starts from fresh gradient buffers (zero on the minibatch's rows, 7.0 elsewhere, or
    `prior`) and NaN loss partials and returns host copies"""

    def __init__(self, dev, case, rows=None, emb=None):
        self.dev, self.c = dev, case
        ru, rp, rn = (case["ru"], case["rp"], case["rn"]) if rows is None else rows
        self.rows = (ru, rp, rn)
        self.ru, self.rp, self.rn = (_t(a, dev, np.int64) for a in (ru, rp, rn))
        self.light, self.light_tab = _t(case["light"], dev), _t(case["light_tab"], dev)
        self.emb = _t(case["emb"] if emb is None else emb, dev)
        self.keys = _t(R.plan_keys(ru, rp, rn).view(np.int64), dev)
        self.touched = np.zeros(case["N"], dtype=bool)
        self.touched[np.concatenate(self.rows)] = True
        self.ops = HipOps()

    def fresh(self, prior=None):
        N, d = self.c["N"], self.c["d"]
        if prior is None:
            g = np.full((N, d), R.SENTINEL, dtype=np.float32)
            g[self.touched] = 0
            prior = (g, g)
        return _t(prior[0], self.dev), _t(prior[1], self.dev), torch.full((_lib.RK_LOSS_PARTIALS,), float("nan"), device=self.dev)

    def ordered(self, L, lam, keys=None):
        gp, ge, lp = self.fresh()
        self.ops.bpr(self.c["d"], L, lam, self.light, self.emb, gp, ge, self.ru, self.rp, self.rn, lp, keys=self.keys if keys is None else keys)
        return gp.cpu().numpy(), ge.cpu().numpy(), lp.cpu().numpy()

    def atomic(self, L, lam, compact=True, prior=None):
        gp, ge, lp = self.fresh(prior)
        if compact:
            self.ops.bpr(self.c["d"], L, lam, self.light, self.emb, gp, ge, self.ru, self.rp, self.rn, lp)
        else:       # the table form: HipOps never asks for it
            _lib.check(_lib.lib().rk_bpr_rows(self.c["d"], L, float(lam), _lib.ptr(self.light_tab), 0, _lib.ptr(self.emb), _lib.ptr(gp), _lib.ptr(ge),
                                              _lib.ptr(self.ru), _lib.ptr(self.rp), _lib.ptr(self.rn), self.c["nb"], _lib.ptr(lp),
                                              _lib.stream_ptr(self.dev)), "rk_bpr_rows")
        return gp.cpu().numpy(), ge.cpu().numpy(), lp.cpu().numpy()


def _check_bpr(entry, touched, ref, bounds, out, prior=None):
    """the assertions every BPR form shares; returns the three ratios"""
    gp, ge, lp = out
    b_gprop, b_gego, b_loss = bounds
    r_gp, r_ge = ref["gprop"], ref["gego"]
    assert np.all(_bits(gp[~touched]) == SENT_BITS) and np.all(_bits(ge[~touched]) == SENT_BITS), "a row outside the minibatch was written"
    if prior is not None:       # (float64 copies of the fp32 prior; 7.0 outside the minibatch like the fresh buffers)
        r_gp, r_ge = r_gp + prior[0], r_ge + prior[1]
        b_gprop, b_gego = b_gprop + R.U32 * np.abs(prior[0]), b_gego + R.U32 * np.abs(prior[1])
    t = touched
    assert lp.shape == (_lib.RK_LOSS_PARTIALS,) and not np.isnan(lp).any(), "a loss partial was not written"
    r = (_ratio(gp[t], r_gp[t], b_gprop[t]), _ratio(ge[t], r_ge[t], b_gego[t]), abs(float(lp.astype(np.float64).sum()) - ref["loss"]) / b_loss)
    _report(f"{entry}.gprop", r[0]); _report(f"{entry}.gego", r[1]); _report(f"{entry}.loss", r[2])
    assert max(r) <= 1.0, r
    return r


@pytest.mark.parametrize("nb,d,L,lam", R.BPR_CASES)
def test_bpr_rows_ordered(gpu_device, bpr_ref, nb, d, L, lam):
    c, ref, bounds = bpr_ref(nb, d, L, lam)
    run = BprRun(gpu_device, c)
    a = run.ordered(L, lam)
    _check_bpr("rk_bpr_rows_ordered", run.touched, ref, bounds, a)
    b = run.ordered(L, lam)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b)), "two runs differ"
    # relabel invariance: other node ids move every run to another place of the plan, another chunk boundary and another wave; a
    # row's incidences keep their (triplet, role) order, so the gradient rows are the same bits at their new places
    N = c["N"]
    perm = np.random.default_rng(nb + d).permutation(N)
    emb2 = np.empty_like(c["emb"])
    emb2[perm] = c["emb"]
    run2 = BprRun(gpu_device, c, rows=tuple(perm[x] for x in run.rows), emb=emb2)
    assert nb < 5 or not np.array_equal(run2.keys.cpu().numpy() >> 20, run.keys.cpu().numpy() >> 20)
    gp2, ge2, lp2 = run2.ordered(L, lam)
    assert np.array_equal(_bits(gp2[perm]), _bits(a[0])) and np.array_equal(_bits(ge2[perm]), _bits(a[1])), "gradient rows depend on the node labels"
    assert not np.isnan(lp2).any() and abs(float(lp2.astype(np.float64).sum()) - ref["loss"]) <= bounds[2]
    # a ragged step: the plan buffer of a larger batch, padded behind the step's own keys as the trainer pads it
    B = nb + 139
    padded = _t(R.pad_keys(np.stack(run.rows), B), gpu_device)
    assert padded.numel() == 3 * B
    r = run.ordered(L, lam, keys=padded)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, r)), "the padded plan of a ragged step changes the result"


def test_bpr_rows_ordered_refusals(gpu_device, bpr_ref):
    c, _, _ = bpr_ref(5, 50, 3, 0.5)
    run = BprRun(gpu_device, c)
    L = _lib.lib()
    for what, over in (("dim > 256", dict(dim=257)), ("3 nb >= 2^20", dict(nb=349526)), ("3 nb >= 2^20", dict(nb=(1 << 20) // 3 + 1)), ("null keys", dict(keys=None)),
                       ("nb = 0", dict(nb=0))):
        a = dict(dim=50, nb=5, keys=run.keys)
        a.update(over)
        gp, ge, lp = run.fresh()
        before = [x.clone() for x in (gp, ge)]
        rc = L.rk_bpr_rows_ordered(a["dim"], 3, 0.5, _lib.ptr(run.light), _lib.ptr(run.emb), _lib.ptr(gp), _lib.ptr(ge), _lib.ptr(run.ru), _lib.ptr(run.rp),
                                   _lib.ptr(run.rn), a["nb"], _lib.ptr(a["keys"]), _lib.ptr(lp), _lib.stream_ptr(gpu_device))
        torch.cuda.synchronize()
        assert rc == EINVAL and L.rk_last_error(), what
        assert torch.equal(gp, before[0]) and torch.equal(ge, before[1]) and bool(torch.isnan(lp).all()), what
    # the largest batch the key format holds is not refused for its size (nothing else about it is valid, so it is not launched here)
    assert 3 * 349525 < (1 << 20) <= 3 * 349526


@pytest.mark.parametrize("nb,d,L,lam", R.BPR_CASES_ATOMIC)
def test_bpr_rows(gpu_device, bpr_ref, nb, d, L, lam):
    c, ref, bounds = bpr_ref(nb, d, L, lam)
    run = BprRun(gpu_device, c)
    a = run.atomic(L, lam, compact=True)
    _check_bpr("rk_bpr_rows[compact]", run.touched, ref, bounds, a)
    t = run.atomic(L, lam, compact=False)
    _check_bpr("rk_bpr_rows[table]", run.touched, ref, bounds, t)
    # `+=`: onto the rows' own gradients (and 7.0 elsewhere), u |prior| more
    prior = (np.where(run.touched[:, None], ref["gprop"], R.SENTINEL).astype(np.float32), np.where(run.touched[:, None], ref["gego"], R.SENTINEL).astype(np.float32))
    p = run.atomic(L, lam, compact=True, prior=prior)
    _check_bpr("rk_bpr_rows[prior]", run.touched, ref, bounds, p, prior=tuple(x.astype(np.float64) for x in prior))
    if d <= 256:    # the ordered and the atomic form: within the sum of their budgets of each other
        o = run.ordered(L, lam)
        tt = run.touched
        for k, name in ((0, "gprop"), (1, "gego")):
            r = _ratio(o[k][tt], a[k][tt].astype(np.float64), 2 * bounds[k][tt])
            _report(f"ordered-vs-atomic.{name}", r)
            assert r <= 1.0
        assert abs(float(o[2].astype(np.float64).sum()) - float(a[2].astype(np.float64).sum())) <= 2 * bounds[2]


# ================================================================ index kernels
GATHER_SHAPES = [(d, n) for d in (1, 7, 64, 100, 256, 300) for n in (1, 3)] + [(7, 16384 + 5)]


def _index_case(d, n, seed):
    """a table whose rows 0..2 hold inf, NaN and negatives, and n indices with duplicates (n > 1) over the other rows"""
    rng = np.random.default_rng(seed)
    rows = 40 if n <= 3 else 20000
    src = rng.standard_normal((rows, d)).astype(np.float32)
    src[0], src[1], src[2] = np.inf, np.nan, -np.abs(src[2]) - 1
    idx = rng.integers(3, rows if n <= 3 else 9000, size=n).astype(np.int64)
    if n >= 3:
        idx[-1] = idx[0]
    return rng, src, idx


@pytest.mark.parametrize("d,n", GATHER_SHAPES)
def test_rows_gather_masked(gpu_device, d, n):
    rng, src, idx = _index_case(d, n, seed=31 * d + n)
    ops = HipOps()
    src_t = _t(src, gpu_device)
    guard = 4
    masks = {"none": None, "mixed": rng.choice(np.array([0.0, 1.0, 0.5], dtype=np.float32), size=n), "zero": np.zeros(n, dtype=np.float32)}
    if n >= 3:
        masks["mixed"][:3] = (0.0, 1.0, 0.5)
    for name, mask in masks.items():
        ix = idx.copy()
        if mask is not None:      # a zero mask entry on the rows holding inf, NaN and negatives: exact +0.0 all the same
            z = np.nonzero(mask == 0)[0]
            ix[z] = np.arange(len(z)) % 3
        out = torch.full((n + guard, d), R.SENTINEL, device=gpu_device)
        ops.gather_rows(src_t, _t(ix, gpu_device), None if mask is None else _t(mask, gpu_device), out[:n])
        got = out.cpu().numpy()
        ref = R.gather_masked(src, ix, mask)
        assert np.array_equal(_bits(got[:n]), _bits(ref)), name
        if mask is not None:
            assert np.all(_bits(got[:n][mask == 0]) == 0), "a zero mask entry must give +0.0"
        assert np.all(_bits(got[n:]) == SENT_BITS), "written past out[n]"
    assert np.array_equal(_bits(src_t.cpu().numpy()), _bits(src))


@pytest.mark.parametrize("d,n", GATHER_SHAPES)
def test_rows_zero(gpu_device, d, n):
    rng, a, idx = _index_case(d, n, seed=37 * d + n)
    b = rng.standard_normal(a.shape).astype(np.float32)
    ops = HipOps()
    for with_b in (True, False):
        at, bt = _t(a, gpu_device), _t(b, gpu_device)
        ops.zero_rows(at, bt if with_b else None, _t(idx, gpu_device))
        assert np.array_equal(_bits(at.cpu().numpy()), _bits(R.zero_rows(a, idx)))         # rows 0..2 (inf, NaN) are not in idx: bits kept
        assert np.array_equal(_bits(bt.cpu().numpy()), _bits(R.zero_rows(b, idx) if with_b else b))
    assert len(np.unique(idx)) < len(idx) or n == 1


@pytest.mark.parametrize("N,n", [(1007, 1), (1007, 300), (50007, 262144 + 77)])
def test_rows_mark_bits(gpu_device, N, n):
    rng = np.random.default_rng(N + n)
    assert N % 32 != 0
    words = (N + 31) // 32
    idx = rng.integers(0, N, size=n).astype(np.int64)
    if n > 1:
        idx[: n // 4] = idx[n // 2]                                      # heavy duplicates
        idx[n // 4: n // 2] = (idx[n // 2] & ~31) + rng.integers(0, 32, size=n // 2 - n // 4)   # many rows of one word
        idx = np.minimum(idx, N - 1)
        idx[-1] = N - 1                                                  # the last, partial word
    ops, idx_t = HipOps(), _t(idx, gpu_device)
    guard = np.uint32(0xDEADBEEF)

    def run(start, on):
        buf = np.append(start, guard).astype(np.uint32)
        t = _t(buf.view(np.int32), gpu_device)
        ops.mark_rows(t, idx_t, on)
        out = t.cpu().numpy().view(np.uint32)
        assert out[-1] == guard, "the word past the bitmap was written"
        return out[:-1]
    empty = np.zeros(words, dtype=np.uint32)
    foreign = rng.integers(0, 1 << 32, size=words, dtype=np.uint64).astype(np.uint32)
    set_empty = run(empty, True)
    assert np.array_equal(set_empty, R.mark_bits(empty, idx, True)) and int(np.unpackbits(set_empty.view(np.uint8)).sum()) == len(np.unique(idx))
    assert np.array_equal(run(foreign, True), R.mark_bits(foreign, idx, True))
    # clear: exactly the words holding an idx bit become 0, foreign bits of those words included; every other word is kept
    cleared = run(foreign, False)
    hit = np.zeros(words, dtype=bool)
    hit[idx >> 5] = True
    assert np.all(cleared[hit] == 0) and np.array_equal(cleared[~hit], foreign[~hit]) and np.array_equal(cleared, R.mark_bits(foreign, idx, False))
    assert (foreign[hit] & ~set_empty[hit]).any(), "the case holds no foreign bit in a cleared word"
    # set then clear with the same indices leaves an empty bitmap empty (the trainers rely on it every step)
    assert not run(set_empty, False).any()


# ================================================================ rk_spmm_csr_ex
class Slab:
    def __init__(self, dev, rect, seed):
        self.dev = dev
        self.csr, self.x_rows = R.spmm_slab(R.SPMM_N, rect, seed)
        self.n = R.SPMM_N
        self.ops = HipOps()
        self.slab = self.ops.make_slab(*self.csr, dev)

    def call(self, d, x, x_rows=None, dim=None, scratch="own", **f):
        """rk_spmm_csr_ex through ctypes (the fields HipOps.spmm does not expose: zero1 / zero2, adam_t < 0, and the refusals) -> rc"""
        desc, n_blocks, scr = HipOps._sched(self.slab, d)
        e = _lib.SpmmEpilogue(sum_scale=float(f.pop("sum_scale", 1.0)), adam_t=int(f.pop("adam_t", 0)), lr=LR, beta1=B1, beta2=B2, eps=EPS)
        for k, v in f.items():
            setattr(e, k, _lib.ptr(v))
        s = self.slab
        return _lib.lib().rk_spmm_csr_ex(self.n, _lib.ptr(s["rowptr"]), _lib.ptr(s["col"]), _lib.ptr(s["val"]), _lib.ptr(desc), n_blocks,
                                         _lib.ptr(scr if scratch == "own" else scratch), d if dim is None else dim, _lib.ptr(x),
                                         x.shape[0] if x_rows is None else x_rows, C.byref(e), _lib.stream_ptr(self.dev))


@pytest.fixture(scope="module")
def slabs(gpu_device):
    memo, refs = {}, {}

    def get(rect, d=None, add=False):
        if rect not in memo:
            memo[rect] = Slab(gpu_device, rect, seed=7 + rect)
        s = memo[rect]
        if d is None:
            return s
        if (rect, d) not in refs:
            refs[rect, d] = {"op": R.spmm_operands(s.n, s.x_rows, d, seed=d)}
        r = refs[rect, d]
        if add not in r:
            op = r["op"]
            r[add] = R.spmm_ex(s.csr, op["x"], op["add"] if add else None, op["sum_in"], op["sum_scale"])
        return s, r["op"], r[add]
    return get


def test_spmm_slabs_reach_every_path(slabs):
    for rect in (False, True):
        s = slabs(rect)
        nnz = np.diff(s.csr[0])
        assert (nnz == 0).sum() >= 2 and nnz.max() == s.x_rows
        for d in R.SPMM_DIMS:
            assert ((nnz > 0) & (nnz <= d // 4)).any() and ((nnz > d // 4) & (nnz <= 100)).any()
            assert HipOps._sched(s.slab, d)[2] is not None, "no long row: the scratch hand-off is not exercised"


@pytest.mark.parametrize("field", list(R.SPMM_FIELDS))
@pytest.mark.parametrize("rect", [False, True])
@pytest.mark.parametrize("d", R.SPMM_DIMS)
def test_spmm_ex_fields(gpu_device, slabs, d, rect, field):
    use_add, use_y, use_sum, use_zero = R.SPMM_FIELDS[field]
    s, op, (v, bv, so, bso) = slabs(rect, d, add=bool(use_add))
    dev, n = gpu_device, s.n
    x = _t(op["x"], dev)
    nan = lambda: torch.full((n, d), float("nan"), device=dev)
    add = _t(op["add"], dev) if use_add else None          # (a fresh copy: the all-together case clears it)
    y = nan() if use_y else None
    sum_in, sum_out = (_t(op["sum_in"], dev), nan()) if use_sum else (None, None)
    z2 = torch.full((n, d), R.SENTINEL, device=dev) if use_zero else None
    z1 = (add if use_add else torch.full((n, d), -R.SENTINEL, device=dev)) if use_zero else None   # all together: the addend is its own zero1
    if use_zero:
        _lib.check(s.call(d, x, add=add, y=y, sum_in=sum_in, sum_out=sum_out, sum_scale=op["sum_scale"], zero1=z1, zero2=z2), "rk_spmm_csr_ex")
    else:
        s.ops.spmm(s.slab, x, add=add, y=y, sum_in=sum_in, sum_out=sum_out, sum_scale=op["sum_scale"])
    if use_y:
        r = _ratio(y.cpu().numpy(), v, bv)
        _report("rk_spmm_csr_ex.y", r)
        assert r <= 1.0
    if use_sum:
        r = _ratio(sum_out.cpu().numpy(), so, bso)
        _report("rk_spmm_csr_ex.sum_out", r)
        assert r <= 1.0
        assert np.array_equal(_bits(sum_in.cpu().numpy()), _bits(op["sum_in"]))
    if use_zero:
        assert np.all(_bits(z1.cpu().numpy()) == 0) and np.all(_bits(z2.cpu().numpy()) == 0), "a zeroed row is not exactly +0.0"
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(op["x"]))


def _adam_state(n, d, dev, seed):
    rng = np.random.default_rng(seed)
    host = (rng.standard_normal((n, d)).astype(np.float32), (0.1 * rng.standard_normal((n, d))).astype(np.float32),
            (rng.random((n, d)) + 0.5).astype(np.float32))
    return host, lambda: {k: _t(a, dev) for k, a in zip("pmv", host)}


def _same(a, b):
    return all(np.array_equal(_bits(a[k].cpu().numpy()), _bits(b[k].cpu().numpy())) for k in "pmv")


@pytest.mark.parametrize("rect", [False, True])
@pytest.mark.parametrize("d", R.SPMM_DIMS)
def test_spmm_ex_adam_needs_no_tolerance(gpu_device, slabs, d, rect):
    """the fused Adam of step t == the same launch into y followed by rk_adam_step(t) on y == the fused form with the coefficients
    already on the device (adam_t < 0), left there by the host (the adam_t > 0 launch) or by rk_adam_coef_advance"""
    s, op, _ = slabs(rect, d, add=True)
    dev, n, t = gpu_device, s.n, 7
    x, add = _t(op["x"], dev), _t(op["add"], dev)
    _, fresh = _adam_state(n, d, dev, seed=d)
    hyp = dict(lr=LR, b1=B1, b2=B2, eps=EPS)
    y = torch.empty(n, d, device=dev)
    s.ops.spmm(s.slab, x, add=add, y=y)
    two = fresh()
    s.ops.adam(two["p"], y, two["m"], two["v"], t, LR, B1, B2, EPS)
    fused, coef = fresh(), torch.zeros(2, device=dev)
    s.ops.spmm(s.slab, x, add=add, adam=dict(fused, t=t, coef=coef, **hyp))
    assert _same(fused, two), "fused Adam differs from SpMM + rk_adam_step"
    host_coef = coef.cpu().numpy()
    replay = fresh()
    _lib.check(s.call(d, x, add=add, adam_t=-1, adam_p=replay["p"], adam_m=replay["m"], adam_v=replay["v"], coef_scratch=coef), "rk_spmm_csr_ex")
    assert _same(replay, two), "adam_t < 0 with the host's coefficients differs"
    assert np.array_equal(_bits(coef.cpu().numpy()), _bits(host_coef)), "adam_t < 0 must not touch coef_scratch"
    dev_coef, counter = torch.full((2,), float("nan"), device=dev), torch.full((1,), t - 1, dtype=torch.int32, device=dev)
    s.ops.adam_advance(dev_coef, counter, LR, B1, B2)
    captured = fresh()
    _lib.check(s.call(d, x, add=add, adam_t=-1, adam_p=captured["p"], adam_m=captured["m"], adam_v=captured["v"], coef_scratch=dev_coef), "rk_spmm_csr_ex")
    assert int(counter.item()) == t and np.array_equal(_bits(dev_coef.cpu().numpy()), _bits(host_coef)), "device and host coefficients of step 7 differ"
    assert _same(captured, two), "adam_t < 0 after rk_adam_coef_advance differs"
    # and the standalone device-coefficient step
    devstep = fresh()
    s.ops.adam(devstep["p"], y, devstep["m"], devstep["v"], t, LR, B1, B2, EPS, coef=dev_coef)
    assert _same(devstep, two)


@pytest.mark.parametrize("d", R.SPMM_DIMS)
def test_spmm_ex_src_filter(gpu_device, slabs, d):
    s = slabs(False)
    dev, n, t = gpu_device, s.n, 3
    rng = np.random.default_rng(500 + d)
    hot = rng.choice(n, n // 10, replace=False)
    hot[0] = 5                                                # the long row's own addend is read on the segment path
    x = np.zeros((n, d), dtype=np.float32)
    x[hot] = rng.standard_normal((len(hot), d)).astype(np.float32)
    sum_in = rng.standard_normal((n, d)).astype(np.float32)
    xt, sin = _t(x, dev), _t(sum_in, dev)
    bits = s.ops.new_row_bits(n, dev)
    s.ops.mark_rows(bits, _t(hot.astype(np.int64), dev), True)
    (p0, m0, v0), fresh = _adam_state(n, d, dev, seed=d + 1)
    hyp = dict(lr=LR, b1=B1, b2=B2, eps=EPS)
    scale = float(np.float32(0.25))

    def launch(filt, add=None, adam=None):
        y, so = torch.full((n, d), float("nan"), device=dev), torch.full((n, d), float("nan"), device=dev)
        s.ops.spmm(s.slab, xt, add=add, y=y, sum_in=sin, sum_out=so, sum_scale=scale, src_filter=bits if filt else None,
                   adam=None if adam is None else dict(adam, t=t, **hyp))
        return y.cpu().numpy(), so.cpu().numpy()
    plain = launch(False)
    st = fresh()
    f1, f2 = launch(True, adam=st), launch(True)
    assert np.array_equal(_bits(f1[0]), _bits(f2[0])) and np.array_equal(_bits(f1[1]), _bits(f2[1])), "two filtered launches differ"
    v, bv, so, bso = R.spmm_ex(s.csr, x, None, sum_in, scale)
    for name, got in (("plain", plain), ("filtered", f1)):
        r = (_ratio(got[0], v, bv), _ratio(got[1], so, bso))
        _report(f"rk_spmm_csr_ex.src_filter[{name}].y", r[0]); _report(f"rk_spmm_csr_ex.src_filter[{name}].sum_out", r[1])
        assert max(r) <= 1.0
    if d in (48, 100):      # no vector kernel: the filter is ignored by design
        assert np.array_equal(_bits(f1[0]), _bits(plain[0])) and np.array_equal(_bits(f1[1]), _bits(plain[1]))
    # the Adam'd parameters of the filtered launch: the bits of rk_adam_step on the filtered y, and within the budget of float64
    two = fresh()
    s.ops.adam(two["p"], _t(f1[0], dev), two["m"], two["v"], t, LR, B1, B2, EPS)
    assert _same(st, two)
    p_ref = R.adam_step(p0, v, m0, v0, t, LR, B1, B2, EPS)[0]
    r = _ratio(st["p"].cpu().numpy(), p_ref, R.adam_param_bound(p0, v, bv, m0, v0, t, LR, B1, B2, EPS))
    _report("rk_spmm_csr_ex.src_filter.adam_p", r)
    assert r <= 1.0
    # add == x, the same pointer (t = A g + g): a row whose bit is clear does not read its addend, which is zero by the contract
    va, bva, soa, bsoa = R.spmm_ex(s.csr, x, x, sum_in, scale)
    a1, a2, a0 = launch(True, add=xt), launch(True, add=xt), launch(False, add=xt)
    assert np.array_equal(_bits(a1[0]), _bits(a2[0])) and np.array_equal(_bits(a1[1]), _bits(a2[1]))
    for name, got in (("plain", a0), ("filtered", a1)):
        r = (_ratio(got[0], va, bva), _ratio(got[1], soa, bsoa))
        _report(f"rk_spmm_csr_ex.add_is_x[{name}].y", r[0]); _report(f"rk_spmm_csr_ex.add_is_x[{name}].sum_out", r[1])
        assert max(r) <= 1.0
    nnz = np.diff(s.csr[0])
    cold = np.setdiff1d(np.arange(n), hot)
    assert ((nnz[cold] > 0) & (nnz[cold] <= d // 4)).any() and (nnz[cold] > d // 4).any() and ((nnz[hot] > 0) & (nnz[hot] <= d // 4)).any()


def test_spmm_ex_refusals(gpu_device, slabs):
    s = slabs(False)
    dev, n, d = gpu_device, s.n, 64
    x = torch.ones(n, d, device=dev)
    bufs = {k: torch.full((n, d), R.SENTINEL, device=dev) for k in ("y", "sum_out", "p", "m", "v")}
    coef = torch.full((2,), R.SENTINEL, device=dev)
    adam = dict(adam_p=bufs["p"], adam_m=bufs["m"], adam_v=bufs["v"], coef_scratch=coef)
    cases = [("sum_out without sum_in", dict(y=bufs["y"], sum_out=bufs["sum_out"])),
             ("a long-row schedule with a null scratch", dict(y=bufs["y"], scratch=None)),
             ("dim > 256", dict(y=bufs["y"], dim=257)), ("dim = 0", dict(y=bufs["y"], dim=0))]
    for missing in adam:
        for t in (1, -1):
            cases.append((f"adam_t = {t} without {missing}", dict({k: v for k, v in adam.items() if k != missing}, y=bufs["y"], adam_t=t)))
    for what, f in cases:
        rc = s.call(d, x, **f)
        torch.cuda.synchronize()
        assert rc == EINVAL and _lib.lib().rk_last_error(), what
        assert all(np.all(_bits(b.cpu().numpy()) == SENT_BITS) for b in list(bufs.values()) + [coef]), what
    _lib.check(s.call(d, x, y=bufs["y"]), "rk_spmm_csr_ex")       # the same call without the fault is taken
    assert not np.any(_bits(bufs["y"].cpu().numpy()) == SENT_BITS)


# ================================================================ rk_adam_coef_advance
def _ulp_apart(got, ref64):
    """|got - ref| in units of the fp32 spacing at ref"""
    return abs(float(got) - ref64) / float(np.spacing(np.float32(ref64)))


@pytest.mark.parametrize("t", [1, 2, 3, 10, 1000, 100000])
def test_adam_coef_advance(gpu_device, t):
    ops = HipOps()
    coef, counter = torch.full((2,), float("nan"), device=gpu_device), torch.full((1,), t - 1, dtype=torch.int32, device=gpu_device)
    ops.adam_advance(coef, counter, LR, B1, B2)
    got, ref = coef.cpu().numpy(), R.adam_coef(t, LR, B1, B2)
    r = max(_ulp_apart(got[0], ref[0]), _ulp_apart(got[1], ref[1]))
    print(f"RATIO rk_adam_coef_advance[ulp] {r:.4f}")
    assert int(counter.item()) == t and r <= 1.0


def test_adam_coef_device_and_host_agree_bit_for_bit_over_4096_steps(gpu_device):
    """the captured step takes its coefficients from rk_adam_coef_advance (pow on the device), the eager step from the host
    (rk_spmm_csr_ex with adam_t = t leaves them in coef_scratch): the trainers' captured-equals-eager claim needs the same bits"""
    dev, T, d = gpu_device, 4096, 32
    ops = HipOps()
    slab = ops.make_slab(np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32), np.array([1.0], dtype=np.float32), dev)
    desc, n_blocks, scr = HipOps._sched(slab, d)
    x = torch.zeros(1, d, device=dev)
    p, m, v = (torch.zeros(1, d, device=dev) for _ in range(3))
    dev_seq, host_seq = torch.full((T, 2), float("nan"), device=dev), torch.full((T, 2), float("nan"), device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    L, stream = _lib.lib(), _lib.stream_ptr(dev)
    e = _lib.SpmmEpilogue(sum_scale=1.0, adam_p=_lib.ptr(p), adam_m=_lib.ptr(m), adam_v=_lib.ptr(v), lr=LR, beta1=B1, beta2=B2, eps=EPS)
    for t in range(1, T + 1):
        rc = L.rk_adam_coef_advance(C.c_void_p(dev_seq.data_ptr() + 8 * (t - 1)), _lib.ptr(counter), LR, B1, B2, stream)
        e.adam_t, e.coef_scratch = t, C.c_void_p(host_seq.data_ptr() + 8 * (t - 1))
        rc |= L.rk_spmm_csr_ex(1, _lib.ptr(slab["rowptr"]), _lib.ptr(slab["col"]), _lib.ptr(slab["val"]), _lib.ptr(desc), n_blocks, _lib.ptr(scr), d,
                               _lib.ptr(x), 1, C.byref(e), stream)
        assert rc == 0, t
    a, b = dev_seq.cpu().numpy(), host_seq.cpu().numpy()        # both sequences read back once
    assert int(counter.item()) == T and not np.isnan(a).any() and not np.isnan(b).any()
    ref = np.array([R.adam_coef(t, LR, B1, B2) for t in range(1, T + 1)])
    assert np.all(np.abs(b - ref) <= np.spacing(ref.astype(np.float32)))
    diff = np.nonzero((_bits(a) != _bits(b)).any(axis=1))[0]
    print(f"steps where the device and host coefficients differ: {len(diff)}" + (f", the first at t = {diff[0] + 1}: {a[diff[0]]} vs {b[diff[0]]}" if len(diff) else ""))
    assert len(diff) == 0
