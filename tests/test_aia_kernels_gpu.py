"""GPU tests of the AIA surrogate kernels one entry point at a time (csrc/aia.hip): each rk_aia_* call on crafted inputs
against the fp64 restatement of tests/_aia_restate.py (itself checked on the CPU by tests/test_aia_host.py), at the pads, batch
sizes, weights and CSR / mask edges where the kernels' loops, shuffles and comparisons change behaviour.  Float outputs are
compared under the first-order error bound computed beside the reference -- no hand-picked tolerance; the only measured numbers
are the expf / logf margins K_ULP and K_EXP_WIDE -- and every bound is asserted to be at most 2^-10 of its tensor's largest
entry.  What must be exact (project, pad columns, untouched rows, a range against its single steps) is compared exactly.

Every output buffer is pre-filled with NaN and carries a sentinel margin after its end.  Each test that claims an edge asserts
that its input has it."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from recad_amd import _lib

from . import _aia_restate as A
from .test_attacker_kernels_gpu import Guarded, _addr
from .test_defender_kernels_gpu import Out, _call, _dev

pytestmark = pytest.mark.gpu
RK_EINVAL = -22
NAN = np.float32(np.nan)


class Desc:
    """rk_aia_desc of a restatement case on the device (the tensors are kept alive here)."""

    def __init__(self, c, dev, **over):
        rowptr = getattr(c, "rowptr", np.zeros(c.R + 1, dtype=np.int32))
        self.rowptr = _dev(np.asarray(rowptr, dtype=np.int32), dev)
        self.col = _addr(getattr(c, "col", []), dev, np.int32)
        self.x = _addr(getattr(c, "x", []), dev, np.float32)
        d = _lib.AiaDesc()
        d.n_rows, d.n_real, d.n_items, d.dpad, d.batch, d.n_fake_nz, d.nnz_real = c.R, c.n_real, c.I, c.dpad, c.batch, c.n_fake_nz, c.nnz_real
        d.rowptr, d.col, d.x = self.rowptr.data_ptr(), self.col.data_ptr(), self.x.data_ptr()
        d.lr, d.beta1, d.beta2, d.eps, d.wd, d.w_pos = c.lr, c.b1, c.b2, c.eps, c.wd, c.w
        for k, v in over.items():
            setattr(d, k, v)
        self.d = d
        self.ref = C.byref(d)


def _slot(case):
    return np.concatenate([case.theta.ravel(), case.m.ravel(), case.v.ravel()])


def _fwd(desc, perm, inv, lo, hi, t_lo, slots, keep_all, parity0, dev):
    L, P, S = _call()
    rc = L.rk_aia_forward(desc.ref, P(perm), P(inv), lo, hi, t_lo, P(slots), keep_all, parity0, S(dev))
    torch.cuda.synchronize()
    return rc


def _rev(desc, perm, inv, lo, hi, t_lo, slots, adj, gbar, xbar, dev):
    L, P, S = _call()
    rc = L.rk_aia_reverse(desc.ref, P(perm), P(inv), lo, hi, t_lo, P(slots), P(adj), P(gbar), P(xbar) if xbar is not None else None, S(dev))
    torch.cuda.synchronize()
    return rc


def _assert_facts(case):
    """The edges a WMF case claims (tests/_aia_restate.py: wmf_case) are in its input."""
    c, f = case.c, A.wmf_facts(case)
    assert f["nb"] == len(case.rows) and f["passes"] == math.ceil(f["nb"] / c.dpad)
    assert f["unrated_item"] and f["has_fake"] and f["zero_fake_ok"]
    if f["nb"] > c.dpad:
        assert f["passes"] >= 2 and f["cross_block"]
    if f["nb"] >= 6:
        assert f["empty_ok"] and f["zero_rating_ok"] and f["first_last"]
    return f


PASSES = {"d16_b40": 3, "d1_b16": 1, "d20_b33": 2, "d32_b32": 1, "d64_b70": 2, "d40_b40": 1, "d16_b256": 16, "last_one": 1, "all_R": 2,
          "betas": 3, "vzero": 3}


# ---------------------------------------------------------------------------------------------------------- project
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_project(gpu_device, n):
    special = np.array([0.5, 1.5, 2.5, 3.5, 4.5, 5.5, -0.5, -1.5, -0.0, 0.0, -3.0, 7.0, 5.0, 4.9999995, 1e30, -1e30, 2.4999998], dtype=np.float32)
    rng = np.random.default_rng(n)
    gen = np.concatenate([special, rng.uniform(-2, 8, max(0, n - len(special))).astype(np.float32)])[:n]
    assert len(gen) == n
    if n > 1:
        assert (np.abs(gen - np.trunc(gen)) == 0.5).sum() >= 6 and (gen < 0).any() and (gen > 5).any() and np.signbit(gen[gen == 0]).any()
    out = Out(n, torch.float32, gpu_device)
    L, P, S = _call()
    _lib.check(L.rk_aia_project(n, P(_dev(gen, gpu_device)), P(out.full), S(gpu_device)), "rk_aia_project")
    torch.cuda.synchronize()
    assert np.array_equal(out.host(), A.project_ref(gen))


def test_project_of_nothing(gpu_device):
    L, _, S = _call()
    assert L.rk_aia_project(0, None, None, S(gpu_device)) == 0
    assert L.rk_aia_g_step(0, None, None, None, None, 1, 1e-2, 0.9, 0.999, 1e-8, S(gpu_device)) == 0


# ---------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("name", list(A.WMF_CASES))
def test_forward_one_step(gpu_device, name):
    case = A.wmf_case(name)
    c = case.c
    f = _assert_facts(case)
    assert f["passes"] == PASSES[name] and c.dpad == A.dpad_of(c.d)
    if name == "last_one":
        assert f["nb"] == 1 and case.j == (c.R + c.batch - 1) // c.batch - 1
    if name == "all_R":
        assert f["nb"] == c.R
    (p1, m1, v1), (pe, me, ve) = A.step_ref(c, case.theta, case.m, case.v, case.perm, case.j, case.adam_t)
    N = (c.R + c.I) * c.dpad
    s0 = _slot(case)
    slots = Guarded(np.concatenate([s0, np.full(6 * N, NAN)]), gpu_device)            # three slots: the step writes the second only
    desc = Desc(c, gpu_device)
    rc = _fwd(desc, _dev(case.perm, gpu_device), _dev(case.invperm, gpu_device), case.j, case.j + 1, case.adam_t, slots.full, 1, 0, gpu_device)
    _lib.check(rc, "rk_aia_forward")
    got = slots.host()
    assert np.array_equal(got[: 3 * N], s0) and np.isnan(got[6 * N:]).all()
    for k, (ref, err) in enumerate(((p1, pe), (m1, me), (v1, ve))):
        g = got[(3 + k) * N:(4 + k) * N].reshape(c.R + c.I, c.dpad)
        assert A.capped(ref, err)
        assert A.within(g, ref, err), (name, k, np.abs(g - ref).max(), float(np.max(np.abs(g - ref) - err)))
        assert not g[:, c.d:].any()                                                  # pad columns stay exactly 0


def test_forward_range_equals_single_steps(gpu_device):
    case = A.wmf_case("d16_b40")
    c = case.c
    N = (c.R + c.I) * c.dpad
    assert (c.R + c.batch - 1) // c.batch == 3
    desc = Desc(c, gpu_device)
    perm, inv = _dev(case.perm, gpu_device), _dev(case.invperm, gpu_device)
    s0 = _slot(case)
    keep = Guarded(np.concatenate([s0, np.full(6 * N, NAN)]), gpu_device)
    _lib.check(_fwd(desc, perm, inv, 1, 3, 7, keep.full, 1, 0, gpu_device), "rk_aia_forward")
    two = Guarded(np.concatenate([s0, np.full(3 * N, NAN)]), gpu_device)
    _lib.check(_fwd(desc, perm, inv, 1, 2, 7, two.full, 0, 0, gpu_device), "rk_aia_forward")
    mid = two.host().copy()
    _lib.check(_fwd(desc, perm, inv, 2, 3, 8, two.full, 0, 1, gpu_device), "rk_aia_forward")
    k, t = keep.host(), two.host()
    assert not np.isnan(k).any()
    assert np.array_equal(mid[3 * N:], k[3 * N:6 * N]) and np.array_equal(mid[: 3 * N], s0)
    assert np.array_equal(t[: 3 * N], k[6 * N:]) and np.array_equal(t[3 * N:], k[3 * N:6 * N])
    # the same two steps as one two-slot range
    rng2 = Guarded(np.concatenate([s0, np.full(3 * N, NAN)]), gpu_device)
    _lib.check(_fwd(desc, perm, inv, 1, 3, 7, rng2.full, 0, 0, gpu_device), "rk_aia_forward")
    assert np.array_equal(rng2.host(), t)


# ---------------------------------------------------------------------------------------------------------- reverse
def _reverse_inputs(case):
    c = case.c
    (p1, m1, v1), _ = A.step_ref(c, case.theta, case.m, case.v, case.perm, case.j, case.adam_t)
    nxt = [a.astype(np.float32) for a in (p1, m1, v1)]
    return np.concatenate([_slot(case)] + [a.ravel() for a in nxt]), nxt


def _check_reverse(case, c, got_adj, got_gbar, got_xbar, ref):
    N = (c.R + c.I) * c.dpad
    got = {"gbar": got_gbar, "adj_th": got_adj[:N], "adj_m": got_adj[N:2 * N], "adj_v": got_adj[2 * N:]}
    for key, g in got.items():
        val, err = ref[key]
        g = g.reshape(c.R + c.I, c.dpad)
        assert np.isfinite(g).all(), key
        assert A.within(g, val, err), (case.name, key, float(np.max(np.abs(g - val) - err)))
        assert not g[:, c.d:].any(), key
        assert A.capped(val, err), key
    if got_xbar is not None:
        inc, err = ref["xbar"]
        want = case.xbar0.astype(np.float64) + inc
        assert np.abs(inc).max() > 0 and A.capped(inc, err)
        assert A.within(got_xbar, want, err + A.U24 * np.abs(want)), (case.name, "xbar")
        assert np.array_equal(got_xbar[inc == 0], case.xbar0[inc == 0])               # entries of rows outside the batch keep their value


@pytest.mark.parametrize("name", list(A.WMF_CASES))
def test_reverse_one_step(gpu_device, name):
    case = A.wmf_case(name)
    c = case.c
    _assert_facts(case)
    slots, (_, m1, v1) = _reverse_inputs(case)
    ref = A.reverse_ref(c, case.theta, m1, v1, *case.adj, case.perm, case.j, case.adam_t)
    N = (c.R + c.I) * c.dpad
    adj = Guarded(np.concatenate([a.ravel() for a in case.adj]), gpu_device)
    gbar, xbar = Out(N, torch.float32, gpu_device), Guarded(case.xbar0, gpu_device)
    assert np.all(case.xbar0 != 0)
    desc = Desc(c, gpu_device)
    rc = _rev(desc, _dev(case.perm, gpu_device), _dev(case.invperm, gpu_device), case.j, case.j + 1, case.adam_t, _dev(slots, gpu_device),
              adj.full, gbar.full, xbar.full, gpu_device)
    _lib.check(rc, "rk_aia_reverse")
    got_adj = adj.host()
    _check_reverse(case, c, got_adj, gbar.host(), xbar.host(), ref)
    if name == "vzero":
        # a row in no batch with zero m and v and wd = 0: g = 0, so m' = v' = 0 and the 1 / sqrt(v') term is taken as 0
        z = case.facts["vzero_row"]
        assert c.wd == 0 and z not in case.rows and not m1[z].any() and not v1[z].any() and case.adj[0][z, : c.d].all()
        a_th, a_v = got_adj[:N].reshape(-1, c.dpad), got_adj[2 * N:].reshape(-1, c.dpad)
        assert np.array_equal(a_v[z], np.float32(c.b2) * case.adj[2][z])              # v-bar = beta2 v-bar': no other term
        assert np.array_equal(a_th[z], case.adj[0][z])                                # theta-bar passes through
        assert np.isfinite(got_adj).all()


def test_reverse_range_equals_single_steps(gpu_device):
    case = A.wmf_case("d20_b33")
    c = case.c
    N = (c.R + c.I) * c.dpad
    assert (c.R + c.batch - 1) // c.batch >= 3 and c.wd == np.float64(0.1)
    desc = Desc(c, gpu_device)
    perm, inv = _dev(case.perm, gpu_device), _dev(case.invperm, gpu_device)
    hist = Guarded(np.concatenate([_slot(case), np.full(6 * N, NAN)]), gpu_device)
    _lib.check(_fwd(desc, perm, inv, 1, 3, 7, hist.full, 1, 0, gpu_device), "rk_aia_forward")
    assert not np.isnan(hist.host()).any()
    outs = []
    for split in (False, True):
        adj = Guarded(np.concatenate([a.ravel() for a in case.adj]), gpu_device)
        gbar, xbar = Out(N, torch.float32, gpu_device), Guarded(case.xbar0, gpu_device)
        if split:
            _lib.check(_rev(desc, perm, inv, 2, 3, 8, hist.full[3 * N:], adj.full, gbar.full, xbar.full, gpu_device), "rk_aia_reverse")
            _lib.check(_rev(desc, perm, inv, 1, 2, 7, hist.full, adj.full, gbar.full, xbar.full, gpu_device), "rk_aia_reverse")
        else:
            _lib.check(_rev(desc, perm, inv, 1, 3, 7, hist.full, adj.full, gbar.full, xbar.full, gpu_device), "rk_aia_reverse")
        outs.append((adj.host().copy(), gbar.host().copy(), xbar.host().copy()))
    for a, b in zip(*outs):
        assert not np.isnan(a).any() and np.array_equal(a, b)
    assert not np.array_equal(outs[0][2], case.xbar0)


def test_reverse_without_fake_entries_takes_a_null_xbar(gpu_device):
    case = A.wmf_case("d32_b32")
    c = case.c
    c.n_real, c.nnz_real, c.n_fake_nz = c.R, int(c.rowptr[c.R]), 0                    # filler_num 0: every row is a rating row
    slots, (_, m1, v1) = _reverse_inputs(case)
    ref = A.reverse_ref(c, case.theta, m1, v1, *case.adj, case.perm, case.j, case.adam_t)
    N = (c.R + c.I) * c.dpad
    adj, gbar = Guarded(np.concatenate([a.ravel() for a in case.adj]), gpu_device), Out(N, torch.float32, gpu_device)
    desc = Desc(c, gpu_device)
    rc = _rev(desc, _dev(case.perm, gpu_device), _dev(case.invperm, gpu_device), case.j, case.j + 1, case.adam_t, _dev(slots, gpu_device),
              adj.full, gbar.full, None, gpu_device)
    _lib.check(rc, "rk_aia_reverse")
    _check_reverse(case, c, adj.host(), gbar.host(), None, ref)


# ---------------------------------------------------------------------------------------------------------- attack loss
def _attack_loss(case, dev, desc=None, **over):
    c = case.c
    N = (c.R + c.I) * c.dpad
    n_p = len(case.pair_user)
    desc = desc or Desc(c, dev)
    a = dict(n_tgt=len(case.tgt), tgt=_dev(case.tgt, dev), ptr=_dev(case.pair_ptr, dev), n_pairs=n_p, user=_dev(case.pair_user, dev),
             ptgt=_dev(case.pair_tgt, dev), slot=_dev(case.pair_slot, dev), pidx=_dev(case.pidx.reshape(-1), dev), scale=_dev(case.tscale, dev),
             theta=_dev(case.theta.ravel(), dev), work=Out(3 * n_p, torch.float32, dev), loss=Out(1, torch.float32, dev),
             adj=Out(3 * N, torch.float32, dev))
    a.update(over)
    L, P, S = _call()
    p = lambda t: None if t is None else P(t.full if isinstance(t, Out) else t)      # noqa: E731
    rc = L.rk_aia_attack_loss(desc.ref, a["n_tgt"], p(a["tgt"]), p(a["ptr"]), a["n_pairs"], p(a["user"]), p(a["ptgt"]), p(a["slot"]),
                              p(a["pidx"]), p(a["scale"]), p(a["theta"]), p(a["work"]), p(a["loss"]), p(a["adj"]), S(dev))
    torch.cuda.synchronize()
    return rc, a


@pytest.mark.parametrize("name", list(A.LOSS_CASES))
def test_attack_loss(gpu_device, name):
    case = A.loss_case(name)
    c = case.c
    n_p = len(case.pair_user)
    assert n_p % 4 and all(n % 4 for n in np.diff(case.pair_ptr))
    if len(case.tgt) > 1:
        assert (case.pidx[:2, 0] >= 0).all() and (case.pidx[:, 1] < 0).all()         # a pair of two targets beside a pair of none
    if name == "ties":
        t0 = int(case.tgt[0])
        assert len(case.dup) == 2 and t0 not in case.dup
        assert all(case.theta[c.R + i].tobytes() == case.theta[c.R + t0].tobytes() for i in case.dup)     # the same bits: an exact fp32 tie
    scores = case.theta[: c.n_real].astype(np.float64) @ case.theta[c.R:].astype(np.float64).T
    assert (scores.max() > 90) == (name == "overflow")
    (loss, le), (adj, ae) = A.attack_loss_ref(*A.loss_args(case), wide=case.wide)
    rc, a = _attack_loss(case, gpu_device)
    _lib.check(rc, "rk_aia_attack_loss")
    N = (c.R + c.I) * c.dpad
    got_loss, got = float(a["loss"].host()[0]), a["adj"].host()
    a["work"].host()                                                                 # scratch: only that writes stay inside 3 n_pairs floats
    assert np.isfinite(got_loss) and np.isfinite(got).all()
    assert A.capped(np.array([loss]), np.array([le])) and abs(got_loss - loss) <= le, (got_loss, loss, le)
    g = got[:N].reshape(c.R + c.I, c.dpad)
    assert A.capped(adj[: c.n_real], ae[: c.n_real]) and A.capped(adj[c.R:], ae[c.R:])
    assert A.within(g, adj, ae), (name, float(np.max(np.abs(g - adj) - ae)))
    assert c.R > c.n_real and not g[c.n_real:c.R].any() and not got[N:].any()         # fake users' rows, m-bar and v-bar: exactly 0
    assert not g[:, c.d:].any()


# ---------------------------------------------------------------------------------------------------------- G step
@pytest.mark.parametrize("n, t", [(1, 1), (256, 1), (257, 1), (1, 1000), (256, 1000), (257, 1000)])
def test_g_step(gpu_device, n, t):
    p, m, v, grads = A.g_case(n, t)
    bufs = [Guarded(a, gpu_device) for a in (p, m, v)]
    L, P, S = _call()
    for k, g in enumerate(grads):
        ref, err = A.g_step_ref(p, m, v, g, 1e-2, 0.9, 0.999, 1e-8, t + k)
        _lib.check(L.rk_aia_g_step(n, *(P(b.full) for b in bufs), P(_dev(g, gpu_device)), t + k, 1e-2, 0.9, 0.999, 1e-8, S(gpu_device)),
                   "rk_aia_g_step")
        torch.cuda.synchronize()
        p, m, v = (b.host().copy() for b in bufs)                                    # the next step starts from the device's own state
        for got, r, e in zip((p, m, v), ref, err):
            assert A.capped(r, e) and A.within(got, r, e), (n, t, k)


# ---------------------------------------------------------------------------------------------------------- refusals
FWD_REFUSALS = {"dpad_48": dict(desc=dict(dpad=48)), "batch_0": dict(desc=dict(batch=0)), "batch_257": dict(desc=dict(batch=257)),
                "n_real_above_n_rows": dict(desc=dict(n_real=101)), "lo_above_hi": dict(lo=2, hi=1), "hi_beyond": dict(lo=1, hi=4),
                "adam_t_0": dict(t=0), "parity_2": dict(parity0=2, keep_all=0), "null_perm": dict(null="perm"), "null_invperm": dict(null="inv"),
                "null_slots": dict(null="slots")}


@pytest.mark.parametrize("what", list(FWD_REFUSALS))
def test_forward_and_reverse_refusals(gpu_device, what):
    case = A.wmf_case("d16_b40")
    c = case.c
    assert c.R == 100 and (c.R + c.batch - 1) // c.batch == 3
    k = dict(dict(desc={}, lo=1, hi=2, t=7, parity0=0, keep_all=1, null=None), **FWD_REFUSALS[what])
    N = (c.R + c.I) * c.dpad
    desc = Desc(c, gpu_device, **k["desc"])
    perm, inv = _dev(case.perm, gpu_device), _dev(case.invperm, gpu_device)
    slots = Guarded(np.concatenate([_slot(case), np.full(3 * N, NAN)]), gpu_device)
    args = {"perm": perm, "inv": inv, "slots": slots.full}
    if k["null"]:
        args[k["null"]] = None
    assert _fwd(desc, args["perm"], args["inv"], k["lo"], k["hi"], k["t"], args["slots"], k["keep_all"], k["parity0"], gpu_device) == RK_EINVAL
    assert np.isnan(slots.host()[3 * N:]).all()                                      # nothing was launched
    if what == "parity_2":
        return
    adj, gbar, xbar = Out(3 * N, torch.float32, gpu_device), Out(N, torch.float32, gpu_device), Out(c.n_fake_nz, torch.float32, gpu_device)
    assert _rev(desc, args["perm"], args["inv"], k["lo"], k["hi"], k["t"], args["slots"], adj.full, gbar.full, xbar.full, gpu_device) == RK_EINVAL
    assert adj.untouched() and gbar.untouched() and xbar.untouched()


@pytest.mark.parametrize("null", ["adj", "gbar", "xbar"])
def test_reverse_refuses_null_outputs(gpu_device, null):
    case = A.wmf_case("d16_b40")
    c = case.c
    N = (c.R + c.I) * c.dpad
    assert c.n_fake_nz > 0
    slots, _ = _reverse_inputs(case)
    bufs = {"adj": Out(3 * N, torch.float32, gpu_device), "gbar": Out(N, torch.float32, gpu_device), "xbar": Out(c.n_fake_nz, torch.float32, gpu_device)}
    a = {k: (None if k == null else b.full) for k, b in bufs.items()}
    L, P, S = _call()
    rc = L.rk_aia_reverse(Desc(c, gpu_device).ref, P(_dev(case.perm, gpu_device)), P(_dev(case.invperm, gpu_device)), 1, 2, 7,
                          P(_dev(slots, gpu_device)), P(a["adj"]), P(a["gbar"]), P(a["xbar"]), S(gpu_device))
    torch.cuda.synchronize()
    assert rc == RK_EINVAL and all(b.untouched() for b in bufs.values())


@pytest.mark.parametrize("what", ["n_tgt", "n_pairs", "tgt", "ptr", "user", "ptgt", "slot", "pidx", "scale", "theta", "work", "loss", "adj", "dpad"])
def test_attack_loss_refusals(gpu_device, what):
    case = A.loss_case("i37_u5")
    over = {what: 0} if what in ("n_tgt", "n_pairs") else ({} if what == "dpad" else {what: None})
    desc = Desc(case.c, gpu_device, dpad=48) if what == "dpad" else None
    rc, a = _attack_loss(case, gpu_device, desc=desc, **over)
    assert rc == RK_EINVAL
    assert all(a[k] is None or a[k].untouched() for k in ("work", "loss", "adj"))


def test_g_step_and_project_refusals(gpu_device):
    L, P, S = _call()
    bufs = [Out(4, torch.float32, gpu_device) for _ in range(4)]
    assert L.rk_aia_g_step(4, *(P(b.full) for b in bufs), 0, 1e-2, 0.9, 0.999, 1e-8, S(gpu_device)) == RK_EINVAL
    assert L.rk_aia_g_step(4, P(bufs[0].full), None, P(bufs[2].full), P(bufs[3].full), 1, 1e-2, 0.9, 0.999, 1e-8, S(gpu_device)) == RK_EINVAL
    assert L.rk_aia_g_step(-1, *(P(b.full) for b in bufs), 1, 1e-2, 0.9, 0.999, 1e-8, S(gpu_device)) == RK_EINVAL
    assert L.rk_aia_project(-1, P(bufs[0].full), P(bufs[1].full), S(gpu_device)) == RK_EINVAL
    assert L.rk_aia_project(4, None, P(bufs[1].full), S(gpu_device)) == RK_EINVAL
    torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs)


# ---------------------------------------------------------------------------------------------------------- the attacker
def test_train_step_against_the_chained_restatement(gpu_device):
    """One train_step at weights the other AIA tests never use (w_pos 0.5, weight decay 0.05, batch 40, d 40 in a pad of
    64): its loss and hypergradient against step_ref / attack_loss_ref / reverse_ref chained in fp64 from entry_state(),
    held to test_aia_gpu's tolerances."""
    from .test_aia_gpu import LOSS_RTOL, _aia, _check_xbar, _synth

    ds, _ = _synth(gpu_device)
    att = _aia(ds, gpu_device, hidden_dim_s=40, batch_size_s=40, weight_pos_s=0.5, weight_decay_s=0.05, epoch_s=2, unroll_steps_s=1)
    assert att.dpad == 64 and att.batch == 40
    x0 = att._x[att.nnz_real:].cpu().numpy().copy()
    targets = [0, 5]
    (loss,) = att.train_step(target_id_list=targets)
    e = att.entry_state()
    R, I, d, dp = att.R, att.n_items, att.dim, att.dpad
    x = att._x.cpu().numpy().copy()
    x[att.nnz_real:] = x0                                                            # the projection the step used
    c = A.SimpleNamespace(R=R, n_real=att.n_users, I=I, d=d, dpad=dp, batch=att.batch, rowptr=att._rowptr.cpu().numpy(), col=att._col.cpu().numpy(),
                          x=x, nnz_real=att.nnz_real, n_fake_nz=att.gen.numel(), lr=att.lr_s, b1=0.9, b2=0.999, eps=1e-8, wd=att.wd_s, w=att.w_pos)

    def padded(P, Q):
        out = np.zeros((R + I, dp))
        out[:R, :d], out[R:, :d] = P, Q
        return out

    th, m, v = padded(e["P"], e["Q"]), padded(e["mP"], e["mQ"]), padded(e["vP"], e["vQ"])
    nsteps, t, hist = (R + att.batch - 1) // att.batch, e["adam_t"], []
    for perm in e["perms"]:
        for j in range(nsteps):
            t += 1
            (th1, m, v), _ = A.step_ref(c, th, m, v, perm, j, t)
            hist.append((th, m, v, perm, j, t))
            th = th1
    pr = att._targets(targets)
    host = lambda k: pr[k].cpu().numpy()      # noqa: E731
    (ref_loss, _), (adj, _) = A.attack_loss_ref(c, th, host("tgt"), host("ptr"), host("user"), host("ptgt"), host("slot"), host("scale"),
                                                   near_ok=True)          # compared under test_aia_gpu's tolerances, not under the bounds
    a_th, a_m, a_v, xbar = adj, np.zeros_like(adj), np.zeros_like(adj), np.zeros(c.n_fake_nz)
    for th_k, m1, v1, perm, j, t in reversed(hist):
        out = A.reverse_ref(c, th_k, m1, v1, a_th, a_m, a_v, perm, j, t)
        a_th, a_m, a_v = out["adj_th"][0], out["adj_m"][0], out["adj_v"][0]
        xbar += out["xbar"][0]
    assert abs(loss - ref_loss) <= LOSS_RTOL * abs(ref_loss), (loss, ref_loss)
    _check_xbar(att.last_hypergradient(), xbar.reshape(att.attack_num, att.filler_num))
