"""GPU tests of the AUSH kernels one entry point at a time (csrc/aush.hip): each rk_aush_* call on crafted inputs against
the restatement of tests/_aush_restate.py (itself checked on the CPU by tests/test_attacker_host.py), at the sizes where the
kernels' loops, ballots and segments change behaviour.  Integer outputs and everything driven by the counter-based draws
are compared exactly; float outputs are compared with fp64 under the first-order error bound computed beside the reference
(no hand-picked tolerance: the only measured number is _aush_restate.K_ULP, the device's expf / logf / log1pf error).  Every
bound is asserted to be at most 2^-10 of its tensor's largest entry, so none can go vacuous.

The gradients are read through the public ABI: with lr = 0, beta1 = beta2 = 0, zero moments and adam_t = 1, rk_aush_d_step
leaves d_m = g exactly, d_v = g * g, and d_param unchanged (include/recad_hip.h).

Every output buffer is pre-filled with NaN (ints: a sentinel) and carries a sentinel margin after its end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset

from . import _aush_restate as R
from .test_defender_kernels_gpu import MARGIN, Out, _call, _dev

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HD, HG = _lib.RK_AUSH_HD, _lib.RK_AUSH_HG
PAD = R.SENTINEL
BYTE = 0xAB


class ByteOut:
    """Out for uint8 outputs: n bytes and a margin, all 0xAB."""

    def __init__(self, n, dev):
        self.n = int(n)
        self.full = torch.full((self.n + MARGIN,), BYTE, dtype=torch.uint8, device=dev)

    def host(self):
        assert (self.full[self.n:].cpu().numpy() == BYTE).all(), "the kernel wrote past the end of its output"
        return self.full[: self.n].cpu().numpy()


class Guarded:
    """An in/out device buffer: the given values followed by a margin of NaN (floats) or -777 (ints), checked on read-back."""

    def __init__(self, a, dev):
        a = np.ascontiguousarray(a)
        self.n, self.fp = a.size, a.dtype.kind == "f"
        pad = np.full(MARGIN, np.nan if self.fp else (BYTE if a.dtype == np.uint8 else -777), dtype=a.dtype)
        self.pad = pad
        self.full = _dev(np.concatenate([a.ravel(), pad]), dev)

    def host(self):
        a = self.full.cpu().numpy()
        tail = a[self.n:]
        assert (np.isnan(tail).all() if self.fp else (tail == self.pad).all()), "the kernel wrote past the end of a buffer"
        return a[: self.n]

    def set(self, a):
        self.full[: self.n] = _dev(np.ascontiguousarray(a).ravel(), self.full.device)


def _csr(rows):
    """(ptr, col, val) from a list of (cols ascending, ratings)."""
    ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(c) for c, _ in rows])
    col = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows] + [np.zeros(0, dtype=np.int32)])
    val = np.concatenate([np.asarray(v, dtype=np.float32) for _, v in rows] + [np.zeros(0, dtype=np.float32)])
    return ptr, col, val


def _addr(a, dev, dtype):
    """A device array that always has an address (one spare element when a is empty)."""
    a = np.asarray(a, dtype=dtype)
    return _dev(a if a.size else np.zeros(1, dtype=dtype), dev)


# ---------------------------------------------------------------------------------------------------------- eligible
def _eligible_case(name):
    """Rows drawn from items [0, 380); the exclusion list lives in [380, 400) plus a few items below; `gone` is a user whose
    whole row is excluded.  Pool sizes are steered to exactly F = 64 (a 64-row; a 65-row with one rating <= 0) and F - 1."""
    rng = np.random.default_rng(sum(map(ord, name)))
    I, F = 400, 64

    def row(n, nonpos=0):
        c = np.sort(rng.choice(380, n, replace=False))
        v = rng.integers(1, 6, n).astype(np.float32)
        if nonpos:
            v[rng.choice(n, nonpos, replace=False)] = rng.choice([0.0, -1.0], nonpos)
        return c, v

    gone = (np.array([381, 385, 399]), np.array([5, 4, 3], dtype=np.float32))
    excl = np.array([381, 385, 390, 399])
    if name == "n1":
        rows = [row(64)]
    elif name == "n3":
        rows = [row(63), row(64), row(0)]
    elif name == "n4":
        rows = [row(65, 1), row(63), row(128), gone]
    elif name == "n5":
        rows = [row(0), row(129), row(64), row(63), gone]
    elif name in ("n257", "no_excl", "nobody"):
        lens = [0, 63, 64, 65, 128, 129, 1, 200]
        rows = [row(lens[u % 8], nonpos=(u % 3) if lens[u % 8] > 3 else 0) for u in range(257)]
        rows[100], rows[256] = gone, row(65, 1)
        if name == "no_excl":
            excl = np.zeros(0, dtype=np.int64)
        if name == "nobody":
            F = 201
    else:
        raise AssertionError(name)
    if len(excl):                                            # excluded items that do occur in the rows
        used = np.unique(np.concatenate([c for c, _ in rows if len(c) and c.max() < 380] + [np.zeros(0, dtype=np.int64)]))
        excl = np.sort(np.concatenate([excl, used[:: max(1, len(used) // 7)][:7]])) if name == "n257" else excl
    return I, F, rows, excl.astype(np.int32)


@pytest.mark.parametrize("name", ["n1", "n3", "n4", "n5", "n257", "no_excl", "nobody"])
def test_eligible(gpu_device, name):
    I, F, rows, excl = _eligible_case(name)
    ptr, col, val = _csr(rows)
    U = len(rows)
    want_ptr, want_col, want_el = R.eligible_ref(ptr, col, val, excl, F)
    sizes = np.diff(want_ptr)
    if name in ("n4", "n5", "n257"):
        assert (sizes == F).any() and (sizes == F - 1).any() and (sizes[[len(c) > 0 for c, _ in rows]] == 0).any()
    if name == "nobody":
        assert len(want_el) == 0
    d_ptr, d_col, d_val = _dev(ptr, gpu_device), _addr(col, gpu_device, np.int32), _addr(val, gpu_device, np.float32)
    d_excl = _dev(excl, gpu_device) if len(excl) else None
    pool_ptr, pool_col, el = Out(U + 1, torch.int32, gpu_device), Out(len(col), torch.int32, gpu_device), Out(U, torch.int32, gpu_device)
    n_el = C.c_int32(-5)
    L, P, S = _call()
    _lib.check(L.rk_aush_eligible(U, P(d_ptr), P(d_col), P(d_val), P(d_excl) if d_excl is not None else None, len(excl), F,
                                  P(pool_ptr.full), P(pool_col.full), P(el.full), C.byref(n_el), S(gpu_device)), "rk_aush_eligible")
    torch.cuda.synchronize()
    assert np.array_equal(pool_ptr.host(), want_ptr)
    got_col, got_el = pool_col.host(), el.host()
    n_pool = int(want_ptr[-1])
    assert np.array_equal(got_col[:n_pool], want_col) and (got_col[n_pool:] == -777).all()
    assert n_el.value == len(want_el)
    assert np.array_equal(got_el[: n_el.value], want_el) and (got_el[n_el.value:] == -777).all()


# ---------------------------------------------------------------------------------------------------------- permute
def _permute(src, n, seed, stream, dev):
    out = Out(n, torch.int32, dev)
    L, P, S = _call()
    _lib.check(L.rk_aush_permute(n, P(src), seed, stream, P(out.full), S(dev)), "rk_aush_permute")
    torch.cuda.synchronize()
    return out.host()


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 5000])
def test_permute(gpu_device, n):
    rng = np.random.default_rng(n)
    src = (rng.permutation(max(n, 1) * 3)[: max(n, 1)] + 7).astype(np.int32)        # distinct, not the identity
    d_src = _dev(src, gpu_device)
    seed, stream = 0x1234ABCD5678, 3
    got = _permute(d_src, n, seed, stream, gpu_device)
    assert np.array_equal(got, src[:n][R.perm_order(n, seed, stream)])
    assert np.array_equal(got, _permute(d_src, n, seed, stream, gpu_device))
    if n >= 255:
        other = _permute(d_src, n, seed, stream + 1, gpu_device)
        assert np.array_equal(other, src[:n][R.perm_order(n, seed, stream + 1)]) and not np.array_equal(other, got)
        assert not np.array_equal(got, src[:n])


# ---------------------------------------------------------------------------------------------------------- sample
def _sample(ptr, col, val, users, F, sel, dev, draws=None, pool=None, seed=0, stream=0, row0=0):
    n, S_ = len(users), len(sel)
    fcol, fval = Out(n * F, torch.int32, dev), Out(n * F, torch.float32, dev)
    nf, sval = Out(n, torch.int32, dev), Out(n * S_, torch.float32, dev)
    keep = [_dev(ptr, dev), _addr(col, dev, np.int32), _addr(val, dev, np.float32), _dev(np.asarray(users, dtype=np.int32), dev),
            _dev(np.asarray(sel, dtype=np.int32), dev)]
    d_draws = _dev(np.asarray(draws, dtype=np.int32), dev) if draws is not None else None
    d_pool = [_dev(pool[0], dev), _addr(pool[1], dev, np.int32)] if pool is not None else [None, None]
    L, P, S = _call()
    _lib.check(L.rk_aush_sample(n, P(keep[3]), F, P(keep[0]), P(keep[1]), P(keep[2]), P(d_pool[0]), P(d_pool[1]), P(d_draws), seed, stream,
                                row0, P(keep[4]), S_, P(fcol.full), P(fval.full), P(nf.full), P(sval.full), S(dev)), "rk_aush_sample")
    torch.cuda.synchronize()
    return fcol.host().reshape(n, F), fval.host().reshape(n, F), nf.host(), sval.host().reshape(n, S_)


def _same_rows(got, want):
    for g, w, what in zip(got, want, ("fcol", "fval", "nf", "sval")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what


@pytest.mark.parametrize("F,n_sel", [(1, 1), (2, 3), (63, 16), (64, 1), (65, 3), (256, 16)])
def test_sample_given_draws(gpu_device, F, n_sel):
    rng = np.random.default_rng(F)
    I, U = 700, 7
    rows = []
    for u in range(U):
        c = np.sort(rng.choice(np.arange(5, 600), 300, replace=False))       # items >= 600 are in nobody's row
        rows.append((c, rng.integers(1, 6, 300).astype(np.float32)))
    ptr, col, val = _csr(rows)
    c0 = rows[0][0]
    # selected: the first and the last item of user 0's row (n_sel >= 3), items nobody rated, and others
    sel = [c0[0]] if n_sel == 1 else [c0[0], c0[-1], 650] + rng.choice(np.arange(5, 600), n_sel - 3, replace=False).tolist()
    sel = np.unique(np.asarray(sel))
    while len(sel) < n_sel:
        sel = np.unique(np.append(sel, rng.integers(5, 700)))
    d = np.empty((U, F), dtype=np.int64)
    half = rows[1][0][rng.permutation(300)[: max(1, F // 2)]]
    d[0] = rows[0][0][17]                                                     # all draws equal: nf = 1
    d[1] = rng.permutation(rows[1][0])[:F]                                    # all distinct
    for r, pick in ((2, half[0]), (3, half[-1]), (4, half.max())):            # repeats of the first / last / largest item
        d[r] = np.concatenate([half, np.full(F - len(half), pick)])[:F] if F > len(half) else half[:F]
    d[5] = rng.choice(np.arange(600, 700), F, replace=F > 100)                # items absent from the row: fval = 0
    d[6] = np.concatenate([rng.permutation(rows[6][0])[: F - F // 3], rng.choice(np.arange(600, 700), F // 3, replace=True)])
    users = np.arange(U)
    want = R.sample_ref(ptr, col, val, users, d, sel)
    assert want[2][0] == 1 and want[2][1] == F and (want[1][5] == 0).all()
    if F >= 63:
        assert want[2][2] < F and (want[0][2, want[2][2]:] == PAD).all()      # a padding tail
    got = _sample(ptr, col, val, users, F, sel, gpu_device, draws=d)
    _same_rows(got, want)
    assert want[3][0, np.searchsorted(sel, c0[0])] == rows[0][1][0]                     # selected items at the row's first position,
    if n_sel >= 3:                                                                    # at its last, and in nobody's row
        assert want[3][0, np.searchsorted(sel, c0[-1])] == rows[0][1][-1] and (want[3][:, np.searchsorted(sel, 650)] == 0).all()


@pytest.mark.parametrize("F", [12, 65])
def test_sample_own_draws(gpu_device, F):
    rng = np.random.default_rng(100 + F)
    I, U = 500, 9
    rows = []
    for u in range(U):
        n = 0 if u == 4 else int(rng.integers(1, 120))
        c = np.sort(rng.choice(I, n, replace=False))
        rows.append((c, np.where(rng.random(n) < 0.1, 0, rng.integers(1, 6, n)).astype(np.float32)))
    ptr, col, val = _csr(rows)
    sel = np.array([3, 250, 499], dtype=np.int32)
    pool_ptr, pool_col, _ = R.eligible_ref(ptr, col, val, np.array([0, 3, 250, 499]), F)
    users = np.array([4, 0, 8, 8, 2, 4, 7], dtype=np.int32)                  # user 4 has an empty pool: nf = 0
    seen = []
    for stream, row0 in ((5, 0), (6, 0), (5, 1000)):
        want = R.sample_ref(ptr, col, val, users, R.own_draws(users, F, pool_ptr, pool_col, 99, stream, row0), sel)
        assert want[2][0] == 0 and (want[0][0] == PAD).all() and want[2][1] > 0
        got = _sample(ptr, col, val, users, F, sel, gpu_device, pool=(pool_ptr, pool_col), seed=99, stream=stream, row0=row0)
        _same_rows(got, want)
        seen.append(got[0])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2])


# ---------------------------------------------------------------------------------------------------------- ZR mask
@pytest.mark.parametrize("n_rows,batch,n_sel,ratio", [(40, 16, 3, 0.2), (40, 16, 3, 0.0), (40, 16, 3, 0.5), (40, 16, 3, 1.0),
                                                      (300, 256, 16, 0.2), (50, 7, 1, 0.5), (5, 64, 2, 0.2)])
def test_zr(gpu_device, n_rows, batch, n_sel, ratio):
    rng = np.random.default_rng(n_rows + n_sel)
    sval = np.where(rng.random((n_rows, n_sel)) < 0.6, 0, rng.integers(1, 6, (n_rows, n_sel))).astype(np.float32)
    sval[:batch] = np.maximum(sval[:batch], 1) if n_rows >= 2 * batch else sval[:batch]   # a batch with no zero pair
    if n_rows >= 2 * batch:
        sval[batch:2 * batch] = 0                                                          # a batch with only zero pairs
    assert n_rows % batch != 0                                                             # the last batch is short
    seed, stream = 77, 2
    want = R.zr_mask(sval, batch, ratio, seed, stream)
    d_sval = _dev(sval, gpu_device)
    zr = ByteOut(n_rows * n_sel, gpu_device)
    L, P, S = _call()
    _lib.check(L.rk_aush_zr(n_rows, batch, n_sel, P(d_sval), ratio, seed, stream, P(zr.full), S(gpu_device)), "rk_aush_zr")
    torch.cuda.synchronize()
    got = zr.host().reshape(n_rows, n_sel)
    assert np.array_equal(got, want)
    assert not got[sval != 0].any()
    if ratio == 0.0:
        assert not got.any()
    if ratio == 1.0:
        assert np.array_equal(got, (sval == 0).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------- generator
@pytest.mark.parametrize("n_sel", [1, 3, 16])
def test_gen(gpu_device, n_sel):
    rng = np.random.default_rng(n_sel)
    I, F, n = 777, 9, 11
    sel = np.unique(np.concatenate([[0, I - 1][: min(2, n_sel)], rng.choice(np.arange(1, I - 1), max(0, n_sel - 2), replace=False)])).astype(np.int32)
    assert len(sel) == n_sel
    fcol = np.full((n, F), PAD, dtype=np.int32)
    fval = np.zeros((n, F), dtype=np.float32)
    nf = np.array([0, 1, F] + rng.integers(0, F + 1, n - 3).tolist(), dtype=np.int32)
    for r in range(n):
        c = np.sort(rng.choice(np.arange(1, I - 1), nf[r], replace=False))
        if nf[r] == F:
            c[0], c[-1] = 0, I - 1                                            # the first and the last item as fillers
        fcol[r, :nf[r]] = c
        fval[r, :nf[r]] = rng.integers(1, 6, nf[r])
    # weights far above torch's range, so that the hidden and the output sigmoids spread over (0, 1)
    w1t, b1 = rng.uniform(-0.3, 0.3, (I, HG)).astype(np.float32), rng.uniform(-1, 1, HG).astype(np.float32)
    w2, b2 = rng.uniform(-0.3, 0.3, (I, HG)).astype(np.float32), rng.uniform(-1, 1, I).astype(np.float32)
    want, bound = R.gen_ref(fcol, fval, nf, w1t, b1, w2, b2, sel, R.K_ULP)
    assert R.capped(want, bound) and np.abs(want - 2.5).max() > 1.0, (bound.max(), want.min(), want.max())   # sigmoids off 0.5
    dv = [_dev(a, gpu_device) for a in (fcol, fval, nf, w1t, b1, w2, b2, sel)]
    gen = Out(n * n_sel, torch.float32, gpu_device)
    L, P, S = _call()
    _lib.check(L.rk_aush_gen(n, F, *[P(t) for t in dv], n_sel, P(gen.full), S(gpu_device)), "rk_aush_gen")
    torch.cuda.synchronize()
    got = gen.host().reshape(n, n_sel)
    print("gen: largest error / bound", np.max(np.abs(got - want) / bound))
    assert R.within(got, want, bound), np.max(np.abs(got - want) / bound)


# ---------------------------------------------------------------------------------------------------------- d_step
class Rig:
    """rk_aush_desc over its own buffers.  The CSR and the generator are not read by rk_aush_d_step; they get small arrays."""

    def __init__(self, I, F, n_sel, batch, sel, P0, dev, lr=0.0, beta1=0.0, beta2=0.0, eps=1e-8, csr=None, G=None):
        self.I, self.F, self.S, self.batch, self.dev = I, F, n_sel, batch, dev
        ptr, col, val = csr if csr is not None else (np.zeros(2, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.float32))
        G = G if G is not None else tuple(np.zeros(n, dtype=np.float32) for n in (HG, HG, HG, 1))
        self.const = [_dev(np.asarray(a), dev) for a in (ptr, col, val, np.asarray(sel, dtype=np.int32), *G)]
        self.n_users = len(ptr) - 1
        self.P0 = np.asarray(P0, dtype=np.float32)
        assert self.P0.size == I * HD + 2 * HD * HD + 4 * HD + 1
        self.p, self.m, self.v = (Guarded(a, dev) for a in (self.P0, np.zeros_like(self.P0), np.zeros_like(self.P0)))
        self.touched, self.n_touched = Guarded(np.zeros(I, dtype=np.uint8), dev), Guarded(np.zeros(1, dtype=np.int32), dev)
        self.touched_list, self.gslot = Out(I, torch.int32, dev), Guarded(np.full(I, -1, dtype=np.int32), dev)
        nb = C.c_int64()
        _lib.check(_lib.lib().rk_aush_workspace_bytes(batch, F, n_sel, C.byref(nb)), "rk_aush_workspace_bytes")
        self.work = torch.full((int(nb.value) + MARGIN,), 0xFF, dtype=torch.uint8, device=dev)   # NaN floats, -1 ints
        d = _lib.AushDesc()
        d.n_users, d.n_items, d.filler_num, d.n_sel, d.batch = self.n_users, I, F, n_sel, batch
        for f, t in zip(("rowptr", "col", "val", "sel", "g_w1t", "g_b1", "g_w2", "g_b2"), self.const):
            setattr(d, f, t.data_ptr())
        for f, t in (("d_param", self.p.full), ("d_m", self.m.full), ("d_v", self.v.full), ("touched", self.touched.full),
                     ("touched_list", self.touched_list.full), ("n_touched", self.n_touched.full), ("gslot", self.gslot.full), ("work", self.work)):
            setattr(d, f, t.data_ptr())
        d.work_bytes = int(nb.value)
        d.lr, d.beta1, d.beta2, d.eps = lr, beta1, beta2, eps
        self.desc = d

    def reset_moments(self):
        """Back to a discriminator that never took a step (the workspace keeps what the last call left in it)."""
        self.m.set(np.zeros_like(self.P0))
        self.v.set(np.zeros_like(self.P0))
        self.touched.set(np.zeros(self.I, dtype=np.uint8))
        self.n_touched.set(np.zeros(1, dtype=np.int32))
        self.touched_list.full.fill_(-777)

    def step(self, c, adam_t=1):
        B = len(c["nf"])
        dv = [_dev(np.ascontiguousarray(c[k]), self.dev) for k in ("fcol", "fval", "nf", "sval", "gen", "zr")]
        losses = Out(4, torch.float32, self.dev)
        L, P, S = _call()
        _lib.check(L.rk_aush_d_step(C.byref(self.desc), B, *[P(t) for t in dv], adam_t, P(losses.full), S(self.dev)), "rk_aush_d_step")
        torch.cuda.synchronize()
        assert (self.work[-MARGIN:] == 0xFF).all(), "a kernel wrote past the end of the workspace"
        return losses.host()


def _check_losses(got, o, what):
    for i in range(4):
        assert o["loss_err"][i] <= 2.0 ** -10 * abs(o["losses"][i]), (what, i)
    print(what, "losses: error / bound", np.abs(got - o["losses"]) / o["loss_err"])
    assert R.within(got, o["losses"], o["loss_err"]), (what, got, o["losses"], o["loss_err"])


def _check_gradient_read_out(rig, c, what):
    """One rk_aush_d_step in the read-out mode (lr = 0, betas = 0, zero moments, adam_t = 1) against d_step_ref."""
    I = rig.I
    o = R.d_step_ref(rig.P0, I, c["fcol"], c["fval"], c["nf"], c["sval"], c["gen"], c["zr"], c["sel"], R.K_ULP)
    assert np.abs(o["z4"]).max() < 10
    got_losses = rig.step(c)
    _check_losses(got_losses, o, what)
    p, m, v = rig.p.host(), rig.m.host(), rig.v.host()
    assert np.array_equal(p.view(np.int32), rig.P0.view(np.int32))               # lr = 0: not one bit of D moves
    items = o["items"]
    n_t = int(rig.n_touched.host()[0])
    assert n_t == len(items) and set(rig.touched_list.host()[:n_t].tolist()) == set(items.tolist())
    assert (rig.touched_list.host()[n_t:] == -777).all()
    assert np.array_equal(rig.touched.host(), np.isin(np.arange(I), items).astype(np.uint8))
    assert (rig.gslot.host() == -1).all()
    gm, gv = R.unpack_d(m, I), R.unpack_d(v, I)
    for k in R.TAIL:
        ref, bound = o["grad"][k], o["grad_err"][k]
        assert R.capped(ref, bound), (what, k)
        got = gm[k].reshape(ref.shape)
        print(what, k, "error / bound", np.max(np.abs(got - ref) / bound))
        assert R.within(got, ref, bound), (what, k, np.max(np.abs(got - ref) / bound))
    assert R.capped(o["gw1"], o["gw1_err"]), what
    print(what, "W1 rows: error / bound", np.max(np.abs(gm["W1t"][items] - o["gw1"]) / np.maximum(o["gw1_err"], 1e-300)))
    assert R.within(gm["W1t"][items], o["gw1"], o["gw1_err"]), what
    rest = np.setdiff1d(np.arange(I), items)
    assert not gm["W1t"][rest].any() and not gv["W1t"][rest].any()               # rows off the batch keep their zeros
    m64 = m.astype(np.float64)
    assert np.all(np.abs(v - m64 * m64) <= 4 * R.U24 * m64 * m64 + 1e-37)        # v = g * g: the same number squared
    return o


D_CASES = [(F, n_sel, B, shared, sel_last) for F, n_sel in ((6, 3), (5, 3)) for B, shared, sel_last in
           ((1, True, True), (2, False, False), (7, False, True), (12, True, False))]


@pytest.mark.parametrize("F,n_sel,B,shared,sel_last", D_CASES)
def test_d_step_gradients(gpu_device, F, n_sel, B, shared, sel_last):
    I, batch = 300, 12                                          # B < batch runs in a workspace sized for batch
    c = R.craft_rows(B, F, n_sel, I, 1000 * F + B, shared=shared, sel_last=sel_last)
    used = set(c["fcol"][c["fcol"] != PAD].tolist()) | set(c["sel"].tolist())
    assert 0 in used and I - 1 in used
    if shared:
        assert all(c["c_all"] in c["fcol"][r, :c["nf"][r]] for r in range(B))      # a filler as frequent as an S item
    else:
        assert (c["nf"] == 0).any()
    if B > 1:
        assert (c["fcol"] == c["c_one"]).sum() == 1 or not c["nf"][0]              # a filler of exactly one row
        assert c["nf"][1] < F
    if sel_last:
        assert c["sel"][-1] == I - 1                                             # the largest id of the batch is selected
    rig = Rig(I, F, n_sel, batch, c["sel"], R.craft_params(I, 7 + B, w=R.CRAFT_W), gpu_device)
    _check_gradient_read_out(rig, c, f"F{F} S{n_sel} B{B}")


def test_d_step_small_batch_after_large(gpu_device):
    """B = 32, then B = 3 on the same descriptor and workspace: nothing of the first call's sorted keys, flags, segment
    starts or gradient rows may reach the second."""
    I, F, n_sel, batch = 300, 6, 3, 32
    c1 = R.craft_rows(32, F, n_sel, I, 5)
    c2 = R.craft_rows(3, F, n_sel, I, 6, shared=False, sel=c1["sel"])
    rig = Rig(I, F, n_sel, batch, c1["sel"], R.craft_params(I, 9, w=R.CRAFT_W), gpu_device)
    _check_gradient_read_out(rig, c1, "B32")
    rig.reset_moments()
    _check_gradient_read_out(rig, c2, "B3 after B32")


def test_d_step_at_the_game_shape(gpu_device):
    """The rows of the first batch of the reference's run on the game data (256 users, 12 draws, S = {62}, 5600 items)."""
    g = np.load(os.path.join(GOLDEN, "aush_game_f12.npz"))
    p = np.load(os.path.join(GOLDEN, "aush_game_partial.npz"))
    ptr, idx, val = dataset.from_config("explicit", "game", train_dict=p["train_kvr"], valid_dict=p["valid_kvr"], test_dict=p["test_kvr"],
                                        device="cpu").rating_csr()
    I, B, F, sel = int(g["n_items"]), int(g["batch_len"][0]), int(g["filler_num"]), np.sort(g["selected_ids"]).astype(np.int32)
    users, draws = g["users"][:B], g["draws"][:B]
    want = R.sample_ref(ptr, idx, val, users, draws, sel)
    got = _sample(ptr.astype(np.int32), idx, val, users, F, sel, gpu_device, draws=draws)
    _same_rows(got, want)
    gen = np.random.default_rng(3).uniform(0.1, 4.9, (B, len(sel))).astype(np.float32)
    c = dict(fcol=want[0], fval=want[1], nf=want[2], sval=want[3], gen=gen, zr=g["zr"][:B].astype(np.uint8), sel=sel)
    rig = Rig(I, F, len(sel), B, sel, R.craft_params(I, 4, w=R.CRAFT_W), gpu_device)
    _check_gradient_read_out(rig, c, "game")


def test_d_step_saturated_output(gpu_device):
    """x rounds to 1 in fp32 (z4 ~ 30): the kernel's documented torch semantics -- x (1 - x) = 0 is clamped to 1e-12 and
    dz4 = gx (1 - x) x is exactly 0, so every gradient is exactly zero; BCE(1, 1) = 0 and BCE(1, 0) is clamped at 100."""
    I, F, n_sel, B = 300, 6, 3, 5
    c = R.craft_rows(B, F, n_sel, I, 8)
    P0 = R.craft_params(I, 3, w=R.CRAFT_W, b4=30.0)
    rig = Rig(I, F, n_sel, 8, c["sel"], P0, gpu_device)
    o = R.d_step_ref(P0, I, c["fcol"], c["fval"], c["nf"], c["sval"], c["gen"], c["zr"], c["sel"])
    assert np.all(np.float32(o["x"]) == 1.0) and np.all(o["z4"] < 40)
    got = rig.step(c)
    assert got[0] == 50.0 and got[3] == 0.0
    assert R.within(got[1:3], o["losses"][1:3], o["loss_err"][1:3])
    assert not rig.m.host().any() and not rig.v.host().any()
    assert np.array_equal(rig.p.host().view(np.int32), P0.view(np.int32))
    assert int(rig.n_touched.host()[0]) == len(o["items"]) and (rig.gslot.host() == -1).all()


def test_d_step_adam_three_steps(gpu_device):
    """Adam itself (default betas, lr 1e-3): three steps, with items touched in step 1, absent in step 2 (g = 0: m and v
    decay, the row still moves) and present again in step 3.  Each step is compared with adam_elem in fp64 started from the
    device's own fp32 state before that step and fed by the restated gradient at those parameters, so every bound is a
    one-step bound; g_loss_gan is restated at the device's updated D."""
    I, F, n_sel, batch = 300, 6, 3, 8
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    c1 = R.craft_rows(8, F, n_sel, I, 31)
    c2 = R.craft_rows(5, F, n_sel, I, 32, shared=False, sel=c1["sel"])
    items = lambda c: set(c["fcol"][c["fcol"] != PAD].tolist()) | set(c["sel"].tolist())
    gone = sorted(items(c1) - items(c2))
    assert len(gone) >= 5 and items(c2) - items(c1)
    rig = Rig(I, F, n_sel, batch, c1["sel"], R.craft_params(I, 33, w=R.CRAFT_W), gpu_device, lr=lr, beta1=b1, beta2=b2, eps=eps)
    ever = set()
    for t, c in enumerate((c1, c2, c1), start=1):
        p0, m0, v0 = (a.host().copy() for a in (rig.p, rig.m, rig.v))
        o = R.d_step_ref(p0, I, c["fcol"], c["fval"], c["nf"], c["sval"], c["gen"], c["zr"], c["sel"], R.K_ULP)
        (pr, mr, vr), (pe, me, ve) = R.adam_ref(p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64), o["g"], o["g_err"],
                                                lr, b1, b2, eps, t)
        got = rig.step(c, adam_t=t)
        p1, m1, v1 = rig.p.host(), rig.m.host(), rig.v.host()
        ever |= items(c)
        never = np.setdiff1d(np.arange(I), sorted(ever))
        for a0, a1 in ((p0, p1), (m0, m1), (v0, v1)):                            # rows never touched: bit-identical
            assert np.array_equal(R.unpack_d(a0, I)["W1t"][never].view(np.int32), R.unpack_d(a1, I)["W1t"][never].view(np.int32))
        for name, a1, ref, err in (("p", p1, pr, pe), ("m", m1, mr, me), ("v", v1, vr, ve)):
            assert R.capped(ref, err), (t, name)
            print("adam step", t, name, "error / bound", np.max(np.abs(a1 - ref) / np.maximum(err, 1e-300)))
            assert R.within(a1, ref, err), (t, name, np.max(np.abs(a1 - ref) / np.maximum(err, 1e-300)))
        if t == 2:                                                               # the absent rows decayed and moved
            w0, w1_ = R.unpack_d(m0, I)["W1t"][gone], R.unpack_d(m1, I)["W1t"][gone]
            assert np.abs(w0).max() > 0 and np.all(np.abs(w1_) <= np.abs(w0)) and np.abs(w1_).max() < np.abs(w0).max()
            assert not np.array_equal(R.unpack_d(p0, I)["W1t"][gone], R.unpack_d(p1, I)["W1t"][gone])
        gan, gan_err = R.gan_loss(p1, I, c["fcol"], c["fval"], c["nf"], c["sval"], c["gen"], c["sel"], R.K_ULP)
        o["losses"][3], o["loss_err"][3] = gan, gan_err
        _check_losses(got, o, f"adam step {t}")
        assert (rig.gslot.host() == -1).all()
    assert int(rig.n_touched.host()[0]) == len(ever)


# ---------------------------------------------------------------------------------------------------------- train_epoch
@pytest.mark.parametrize("batch", [16, 64])
def test_train_epoch_equals_its_pieces(gpu_device, batch):
    """rk_aush_train_epoch against rk_aush_permute, _sample, _zr, _gen and one rk_aush_d_step per batch from the same state:
    bit-identical (no float atomics anywhere).  N is not a multiple of 16, and below 64."""
    dev = gpu_device
    rng = np.random.default_rng(batch)
    I, U, F, n_sel = 300, 45, 6, 3
    rows = []
    for u in range(U):
        n = int(rng.integers(2, 40))
        cc = np.sort(rng.choice(I, n, replace=False))
        rows.append((cc, rng.integers(1, 6, n).astype(np.float32)))
    ptr, col, val = _csr(rows)
    sel = np.array([10, 150, 299], dtype=np.int32)
    excl = np.array([0, 10, 150, 299], dtype=np.int32)
    pool_ptr, pool_col, el = R.eligible_ref(ptr, col, val, excl, F)
    N = len(el)
    assert N % 16 != 0 and 16 < N < 64
    G = (rng.uniform(-0.3, 0.3, (I, HG)).astype(np.float32), rng.uniform(-1, 1, HG).astype(np.float32),
         rng.uniform(-0.3, 0.3, (I, HG)).astype(np.float32), rng.uniform(-1, 1, I).astype(np.float32))
    P0 = R.craft_params(I, 50, w=1.0, b4=0.0)
    seed, epoch, ratio, t0 = 4242, 3, 0.2, 5
    nb = (N + batch - 1) // batch
    d_el, d_pp, d_pc = _dev(el, dev), _dev(pool_ptr, dev), _dev(pool_col, dev)
    L, P, S = _call()

    def buffers():
        return dict(perm=Out(N, torch.int32, dev), fcol=Out(N * F, torch.int32, dev), fval=Out(N * F, torch.float32, dev), nf=Out(N, torch.int32, dev),
                    sval=Out(N * n_sel, torch.float32, dev), gen=Out(N * n_sel, torch.float32, dev), zr=ByteOut(N * n_sel, dev),
                    losses=Out(nb * 4, torch.float32, dev))

    a, ra = buffers(), Rig(I, F, n_sel, batch, sel, P0, dev, lr=1e-3, beta1=0.9, beta2=0.999, csr=(ptr, col, val), G=G)
    _lib.check(L.rk_aush_train_epoch(C.byref(ra.desc), P(d_el), N, P(d_pp), P(d_pc), seed, epoch, ratio, t0, *[P(a[k].full) for k in
                                     ("perm", "fcol", "fval", "nf", "sval", "gen", "zr", "losses")], S(dev)), "rk_aush_train_epoch")
    torch.cuda.synchronize()
    b, rb = buffers(), Rig(I, F, n_sel, batch, sel, P0, dev, lr=1e-3, beta1=0.9, beta2=0.999, csr=(ptr, col, val), G=G)
    k = rb.const
    _lib.check(L.rk_aush_permute(N, P(d_el), seed, epoch, P(b["perm"].full), S(dev)), "rk_aush_permute")
    _lib.check(L.rk_aush_sample(N, P(b["perm"].full), F, P(k[0]), P(k[1]), P(k[2]), P(d_pp), P(d_pc), None, seed, epoch, 0, P(k[3]), n_sel,
                                P(b["fcol"].full), P(b["fval"].full), P(b["nf"].full), P(b["sval"].full), S(dev)), "rk_aush_sample")
    _lib.check(L.rk_aush_zr(N, batch, n_sel, P(b["sval"].full), ratio, seed, epoch, P(b["zr"].full), S(dev)), "rk_aush_zr")
    _lib.check(L.rk_aush_gen(N, F, P(b["fcol"].full), P(b["fval"].full), P(b["nf"].full), P(k[4]), P(k[5]), P(k[6]), P(k[7]), P(k[3]), n_sel,
                             P(b["gen"].full), S(dev)), "rk_aush_gen")
    for i in range(nb):
        r0, B = i * batch, min(batch, N - i * batch)
        view = lambda key, w: b[key].full[r0 * w:]
        _lib.check(L.rk_aush_d_step(C.byref(rb.desc), B, P(view("fcol", F)), P(view("fval", F)), P(view("nf", 1)), P(view("sval", n_sel)),
                                    P(view("gen", n_sel)), P(view("zr", n_sel)), t0 + i + 1, P(b["losses"].full[4 * i:]), S(dev)), "rk_aush_d_step")
    torch.cuda.synchronize()
    for key in ("perm", "fcol", "fval", "nf", "sval", "gen", "zr", "losses"):
        x, y = a[key].host(), b[key].host()
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), key
    assert np.isfinite(a["losses"].host()).all()
    assert np.array_equal(np.sort(a["perm"].host()), el)
    assert np.array_equal(a["zr"].host().reshape(N, n_sel), R.zr_mask(a["sval"].host().reshape(N, n_sel), batch, ratio, seed, epoch))
    for x, y in ((ra.p, rb.p), (ra.m, rb.m), (ra.v, rb.v), (ra.touched, rb.touched), (ra.n_touched, rb.n_touched)):
        assert np.array_equal(x.host().view(np.uint8), y.host().view(np.uint8))
    assert not np.array_equal(ra.p.host(), P0) and np.isfinite(ra.p.host()).all()


# ---------------------------------------------------------------------------------------------------------- fake_assemble
@pytest.mark.parametrize("n_rows,with_targets", [(1, False), (50, True), (50, False), (1, True)])
def test_fake_assemble(gpu_device, n_rows, with_targets):
    rng = np.random.default_rng(n_rows)
    I, F = 333, 5                                               # not a multiple of 64
    sel = np.array([0, 40, 41, 332], dtype=np.int32)
    tgt = np.array([7, 41, 300], dtype=np.int32) if with_targets else np.zeros(0, dtype=np.int32)   # 41 is selected too
    pool = np.setdiff1d(np.arange(I), np.concatenate([sel, tgt]))
    fcol = np.full((n_rows, F), PAD, dtype=np.int32)
    fval = np.zeros((n_rows, F), dtype=np.float32)
    nf = rng.integers(0, F + 1, n_rows).astype(np.int32)
    nf[0] = F
    for r in range(n_rows):
        fcol[r, :nf[r]] = np.sort(rng.choice(pool, nf[r], replace=False))
        fval[r, :nf[r]] = rng.integers(1, 6, nf[r])
    gen = rng.uniform(0, 5, (n_rows, 4)).astype(np.float32)
    gen[0] = [2.5, 3.5, 0.5, 4.5]                               # ties: 2, 4, 0 -> clipped to 1, 4
    dv = [_dev(a, gpu_device) for a in (fcol, fval, nf, sel)]
    d_gen, d_tgt = _dev(gen, gpu_device), (_dev(tgt, gpu_device) if with_targets else None)
    out = Out(n_rows * I, torch.float32, gpu_device)
    pre = Out(n_rows * 4, torch.float32, gpu_device) if with_targets else None       # pre == NULL is accepted
    L, P, S = _call()
    _lib.check(L.rk_aush_fake_assemble(n_rows, I, F, P(dv[0]), P(dv[1]), P(dv[2]), P(dv[3]), 4, P(d_gen), P(d_tgt) if with_targets else None,
                                       len(tgt), P(pre.full) if pre else None, P(out.full), S(gpu_device)), "rk_aush_fake_assemble")
    torch.cuda.synchronize()
    v = gen + np.where(np.isin(sel, tgt), np.float32(5), np.float32(0))[None, :]
    want = np.zeros((n_rows, I), dtype=np.float32)
    for r in range(n_rows):
        want[r, fcol[r, :nf[r]]] = fval[r, :nf[r]]
    want[:, tgt] = 5
    want[:, sel] = np.clip(np.rint(v), 1, 5)
    assert want[0, sel].tolist() == ([2, 4, 5, 4] if with_targets else [2, 4, 1, 4])
    assert np.array_equal(out.host().reshape(n_rows, I), want)
    if pre:
        assert np.array_equal(pre.host().reshape(n_rows, 4), v)
