"""Every form of the LDS-resident SpMM (recad_amd/csrc/spmm_lds.h) on the device, bit for bit against the walk of its own plan
(tests/_lds_restate.py).  The shipped planner only ever picks (lpa, lpb) = (1, 1) with chunk cap 64; the plans here are built by
rk_lds_plan_build_host_ex, uploaded by rk_lds_plan_upload and launched through rk_spmm_lds (and, seeded into a graph's plan cache,
through the LightGCN handle: the staged hand-off between layers and the multi-phase launch).  The same cases pass
tests/test_spmm_lds_forms_host.py on the CPU first: the walk covers every entry once, meets its rounding budget against the
float64 product, and the multi-phase queues cannot deadlock.

Contracts (u = 2^-24):
  no addend      y == fl(acc * dinv[r]) of the walk, np.array_equal -- "every sum has a fixed order"; nothing can contract
  addend         |got - (acc dinv + add)| <= u (|acc dinv| + |acc dinv + add|): the scale and the add may or may not be one FMA
  running sum    sum_out == fl(fl(sum_in + y_got) * scale) when y is requested too; the addend budget + 2u (|sum_in| + |v|) |scale| if not
  Adam           p / m / v == the oracle's Adam on the kernel's own y, bit for bit; shadow == the sliced copy of p
Every output sits behind sentinel guards; what is not requested keeps its sentinel; every launch is repeated and must repeat."""
import ctypes as C

import numpy as np
import pytest
import torch

from recad_amd import _lib
from tests import _lds_restate as R
from tests._gemm_forms import SENT, Guarded

pytestmark = pytest.mark.gpu

_dev_plans, _sl_idx = {}, {}


def _upload(dev, graph, dim, n_cu, form, cap):
    plan, info, rc, n_words = R.build_plan_handle(*graph, dim, n_cu, form, cap)
    assert rc == 0 and plan is not None, _lib.lib().rk_last_error()
    try:
        words = R.plan_words(plan, n_words)
        buf = torch.zeros(n_words + 4, device=dev, dtype=torch.int32)
        buf = buf[((-buf.data_ptr() // 4) % 4):][:n_words]   # 16-byte aligned view
        _lib.check(_lib.lib().rk_lds_plan_upload(plan, _lib.ptr(buf), _lib.stream_ptr()), "rk_lds_plan_upload")
    finally:
        _lib.lib().rk_lds_plan_destroy(plan)
    assert np.array_equal(buf.cpu().numpy(), words)
    return buf, info, words


def _plan(dev, case):
    if case not in _dev_plans:
        g, dim, n_cu, form, cap = case
        _dev_plans[case] = _upload(dev, R.case_graph(g), dim, n_cu, R.FORMS[form], cap)
    return _dev_plans[case]


def _idx(info):
    key = bytes(info)
    if key not in _sl_idx:
        _sl_idx[key] = R.sl_index(info)
    return _sl_idx[key]


def _sliced(info, rm):
    out = np.empty(rm.size, dtype=np.float32)
    out[_idx(info).ravel()] = rm.ravel()
    return out


def _rowmajor(info, sl):
    return sl[_idx(info)]


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _launch(info, plan, xs, **fields):
    fields.setdefault("sum_scale", 1.0)
    epi = _lib.LdsEpilogue(**fields)
    rc = _lib.lib().rk_spmm_lds(C.byref(info), _lib.ptr(plan) if isinstance(plan, torch.Tensor) else plan, _lib.ptr(xs), C.byref(epi), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _twice(run):
    """run() -> tuple of arrays; every case runs twice and must repeat bit for bit"""
    a, b = run(), run()
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "not reproducible run to run"
    return a


def _as_rm(info, got, rm):
    N, d = info.n_users + info.n_items, info.dim
    return got.reshape(N, d) if rm else _rowmajor(info, got)


# seven forms on the graph with every row length, plus the shapes with several blocks / the staging loop's second trip
SUB = [("edge", 16, 8, f, 0) for f in R.FORMS] + [("edge_t", 48, 256, (2, 4), 0), ("edge_t", 16, 2, (4, 2), 0), ("edge", 16, 8, (4, 4), 512),
                                                   ("long2", 8, 256, (1, 2), 0), ("three", 16, 8, (2, 1), 0)]
assert set(SUB) <= set(R.CASES)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_no_addend_equals_the_walk_bit_for_bit(gpu_device, case):
    plan, info, _ = _plan(gpu_device, case)
    w = R.case_walk(case)
    N, d = w.y0.shape
    xs = _t(gpu_device, _sliced(info, R.case_x(case)))
    for rm in (0, 1):
        def run():
            y = Guarded(gpu_device, N * d)
            assert _launch(info, plan, xs, y=y.ptr, y_row_major=rm) == 0, _lib.lib().rk_last_error()
            got = y.read().copy()
            assert y.untouched()
            return (got,)
        (got,) = _twice(run)
        got = _as_rm(info, got, rm)
        bad = got != w.y0
        assert not bad.any(), (rm, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], w.y0[bad][:4])


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_addend_within_two_roundings(gpu_device, case):
    """The scale and the add may legally contract into one FMA: neither is demanded, both are within the budget.  Which one the
    build took is printed (measured with this build: bit-equal to the FUSED form, fl(acc * dinv + add), in every case of every
    pair, sliced and row-major; worst budget ratio 0.995)."""
    plan, info, _ = _plan(gpu_device, case)
    w = R.case_walk(case)
    N, d = w.y0.shape
    add = R.case_x(case, "add")
    xs, adds = _t(gpu_device, _sliced(info, R.case_x(case))), _t(gpu_device, _sliced(info, add))
    exact, bud = R.addend_budget(w, add)
    for rm in (0, 1):
        def run():
            y = Guarded(gpu_device, N * d)
            assert _launch(info, plan, xs, add=_lib.ptr(adds), y=y.ptr, y_row_major=rm) == 0, _lib.lib().rk_last_error()
            got = y.read().copy()
            assert y.untouched()
            return (got,)
        (got,) = _twice(run)
        got = _as_rm(info, got, rm)
        err = np.abs(got.astype(np.float64) - exact)
        ratio = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bud, 1e-300))))
        sep, fus = np.array_equal(got, R.addend_separate(w, add)), np.array_equal(got, R.addend_fused(w, add))
        print(f"{R.case_id(case)} rm={rm}: addend budget ratio {ratio:.3f}, bit-equal to separate {sep}, to fused {fus}")
        assert (err <= bud).all(), (rm, ratio)
    assert torch.equal(adds, _t(gpu_device, _sliced(info, add)))       # the addend is only read


@pytest.mark.parametrize("case", SUB, ids=R.case_id)
def test_running_sum_both_layouts(gpu_device, case):
    """sum_out = (sum_in + v) * scale, sliced and row-major, scales 1, 0.25 and 1/3; with and without y, with and without an
    addend (no addend: v is the walk's y0 exactly, so sum_out is exact even with y NULL)."""
    plan, info, _ = _plan(gpu_device, case)
    w = R.case_walk(case)
    N, d = w.y0.shape
    add, s_in = R.case_x(case, "add"), R.case_x(case, "sum_in")
    xs, adds, sins = (_t(gpu_device, _sliced(info, a)) for a in (R.case_x(case), add, s_in))
    exact, bud = R.addend_budget(w, add)
    for sum_rm in (0, 1):
        for scale in (1.0, 0.25, 1.0 / 3.0):
            for with_add in (True, False):
                def run(with_y):
                    y, so = Guarded(gpu_device, N * d), Guarded(gpu_device, N * d)
                    rc = _launch(info, plan, xs, add=_lib.ptr(adds) if with_add else None, y=y.ptr if with_y else None, sum_in=_lib.ptr(sins),
                                 sum_out=so.ptr, sum_out_row_major=sum_rm, sum_scale=scale)
                    assert rc == 0, _lib.lib().rk_last_error()
                    gy, gs = y.read().copy(), so.read().copy()
                    assert so.untouched() and (y.untouched() if with_y else y.untouched(np.zeros(N * d, dtype=bool)))
                    return gy, gs
                gy, gs = _twice(lambda: run(True))
                gy, gs = _rowmajor(info, gy), _as_rm(info, gs, sum_rm)
                assert np.array_equal(gs, R.running_sum(s_in, gy, scale)), (sum_rm, scale, with_add)
                if not with_add:
                    assert np.array_equal(gy, w.y0)
                _, gs2 = _twice(lambda: run(False))
                gs2 = _as_rm(info, gs2, sum_rm)
                if with_add:
                    want = (s_in.astype(np.float64) + exact) * float(np.float32(scale))
                    assert (np.abs(gs2 - want) <= R.running_sum_budget(s_in, bud, exact, scale)).all(), (sum_rm, scale)
                else:
                    assert np.array_equal(gs2, R.running_sum(s_in, w.y0, scale)), (sum_rm, scale)
    assert torch.equal(sins, _t(gpu_device, _sliced(info, s_in)))


@pytest.mark.parametrize("case", SUB, ids=R.case_id)
def test_zeroing_also_of_the_addend_itself(gpu_device, case):
    """zero1 / zero2 become exact zeros; zero1 may be the addend's own buffer (the train step's use: the kernel reads the addend
    before it clears it) -- same result as with a separate buffer."""
    plan, info, _ = _plan(gpu_device, case)
    N, d = R.case_walk(case).y0.shape
    add = _sliced(info, R.case_x(case, "add"))
    xs = _t(gpu_device, _sliced(info, R.case_x(case)))

    def run(alias):
        y, z1, z2 = Guarded(gpu_device, N * d), Guarded(gpu_device, N * d, fill=add), Guarded(gpu_device, N * d)
        a = z1 if alias else Guarded(gpu_device, N * d, fill=add)
        assert _launch(info, plan, xs, add=a.ptr, y=y.ptr, zero1=z1.ptr, zero2=z2.ptr) == 0, _lib.lib().rk_last_error()
        gy, g1, g2 = y.read().copy(), z1.read().copy(), z2.read().copy()
        assert y.untouched() and z1.untouched() and z2.untouched()
        assert not g1.view(np.uint32).any() and not g2.view(np.uint32).any()      # +0.0, every element
        if not alias:
            assert np.array_equal(a.read(), add) and a.untouched()
        return (gy,)
    (sep,), (ali,) = _twice(lambda: run(False)), _twice(lambda: run(True))
    assert np.array_equal(sep.view(np.uint32), ali.view(np.uint32))
    # only one of the two
    y, z2 = Guarded(gpu_device, N * d), Guarded(gpu_device, N * d)
    assert _launch(info, plan, xs, y=y.ptr, zero2=z2.ptr) == 0
    assert not z2.read().view(np.uint32).any() and z2.untouched()


@pytest.mark.parametrize("case", SUB[:7] + SUB[-2:], ids=R.case_id)
def test_adam_epilogue_equals_the_oracle_on_the_kernels_own_gradient(gpu_device, case):
    """adam_t 1, 3, 1000, with and without shadow: p / m / v (row-major) are the oracle's Adam applied to the y this launch
    wrote, bit for bit (common.h: every operation of adam_elem is rounded on its own, like the oracle's)."""
    plan, info, _ = _plan(gpu_device, case)
    N, d = R.case_walk(case).y0.shape
    rng = np.random.default_rng(N * d)
    p0 = rng.standard_normal((N, d)).astype(np.float32)
    m0 = (0.01 * rng.standard_normal((N, d))).astype(np.float32)
    v0 = (0.001 * rng.random((N, d))).astype(np.float32)
    xs, adds = (_t(gpu_device, _sliced(info, a)) for a in (R.case_x(case), R.case_x(case, "add")))
    for t in (1, 3, 1000):
        for with_shadow in (True, False):
            def run():
                y, sh = Guarded(gpu_device, N * d), Guarded(gpu_device, N * d)
                p, m, v = (Guarded(gpu_device, N * d, fill=a.ravel()) for a in (p0, m0, v0))
                coef = Guarded(gpu_device, 4)
                rc = _launch(info, plan, xs, add=_lib.ptr(adds), y=y.ptr, y_row_major=1, adam_t=t, adam_p=p.ptr, adam_m=m.ptr, adam_v=v.ptr,
                             adam_shadow=sh.ptr if with_shadow else None, coef_scratch=coef.ptr, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
                assert rc == 0, _lib.lib().rk_last_error()
                out = tuple(b.read().copy() for b in (y, p, m, v, sh))
                assert all(b.untouched() for b in (y, p, m, v)) and (sh.untouched() if with_shadow else sh.untouched(np.zeros(N * d, dtype=bool)))
                coef.read()
                assert coef.untouched(np.asarray([True, True, False, False]))
                return out
            gy, gp, gm, gv, gsh = _twice(run)
            rp, rm_, rv = R.adam(p0, m0, v0, gy.reshape(N, d), t)
            for name, got, ref in (("m", gm, rm_), ("v", gv, rv), ("p", gp, rp)):
                bad = got.reshape(N, d) != ref
                assert not bad.any(), (name, t, int(bad.sum()), got.reshape(N, d)[bad][:3], ref[bad][:3])
            if with_shadow:
                assert np.array_equal(gsh, _sliced(info, gp))


@pytest.mark.parametrize("case", [("edge", 16, 8, (1, 2), 0), ("edge_t", 48, 256, (2, 4), 0), ("edge", 16, 8, (4, 2), 0), ("three", 16, 8, (2, 1), 0),
                                  ("edge", 16, 8, (1, 1), 0)], ids=R.case_id)
def test_pack_and_unpack_several_arrays_with_gaps(gpu_device, case):
    """rk_lds_pack / rk_lds_unpack loop over their arrays in threes: 1, 3, 4 and 7 arrays, a stride larger than the array; the
    gaps keep their sentinel, the layout is sl_off's (users and items blocks sliced differently), the round trip is exact."""
    _, info, _ = _plan(gpu_device, case)
    assert case[3][0] == case[3][1] or info.lsu != info.lsi
    N, d = info.n_users + info.n_items, info.dim
    n, stride = N * d, N * d + 20
    rng = np.random.default_rng(n)
    L = _lib.lib()
    for n_arrays in (1, 3, 4, 7):
        total = (n_arrays - 1) * stride + n
        data = rng.standard_normal((n_arrays, N, d)).astype(np.float32)
        fill = np.full(total, SENT, dtype=np.float32)
        payload = np.zeros(total, dtype=bool)
        for q in range(n_arrays):
            fill[q * stride: q * stride + n] = data[q].ravel()
            payload[q * stride: q * stride + n] = True
        src, sl, back = Guarded(gpu_device, total, fill=fill), Guarded(gpu_device, total), Guarded(gpu_device, total)
        _lib.check(L.rk_lds_pack(C.byref(info), src.ptr, sl.ptr, n_arrays, stride, _lib.stream_ptr()), "rk_lds_pack")
        _lib.check(L.rk_lds_unpack(C.byref(info), sl.ptr, back.ptr, n_arrays, stride, _lib.stream_ptr()), "rk_lds_unpack")
        torch.cuda.synchronize()
        gs, gb = sl.read().copy(), back.read().copy()
        assert sl.untouched(payload) and back.untouched(payload)
        assert np.array_equal(src.read(), fill) and src.untouched()
        for q in range(n_arrays):
            assert np.array_equal(gs[q * stride: q * stride + n], R.to_sliced(info, data[q])), (n_arrays, q)
            assert np.array_equal(gb[q * stride: q * stride + n], data[q].ravel()), (n_arrays, q)


def test_refusals_launch_nothing(gpu_device):
    """sum_out without sum_in, missing Adam pointers, zeroed info, a (1, 4) plan (no instantiation), an unaligned plan pointer:
    an error code, and every output keeps its sentinel."""
    case = ("edge", 16, 8, (2, 2), 0)
    plan, info, _ = _plan(gpu_device, case)
    N, d = info.n_users + info.n_items, info.dim
    xs = _t(gpu_device, _sliced(info, R.case_x(case)))
    graph = R.case_graph("edge")
    plan14, info14, _ = _upload(gpu_device, graph, 16, 8, (4, 16), 0)
    assert (info14.lpa, info14.lpb) == (1, 4)
    x14 = _t(gpu_device, R.to_sliced(info14, R.case_x(case)))
    outs = [Guarded(gpu_device, N * d) for _ in range(6)]
    y, so, p, m, v, sh = outs
    coef = Guarded(gpu_device, 4)
    adam = dict(adam_t=3, adam_m=m.ptr, adam_v=v.ptr, adam_shadow=sh.ptr, coef_scratch=coef.ptr, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    for what, rc in (
            ("sum_out without sum_in", _launch(info, plan, xs, y=y.ptr, sum_out=so.ptr)),
            ("Adam without p", _launch(info, plan, xs, y=y.ptr, **adam)),
            ("Adam without its coefficient scratch", _launch(info, plan, xs, y=y.ptr, **dict(adam, adam_p=p.ptr, coef_scratch=None))),
            ("zeroed info", _launch(_lib.LdsInfo(), plan, xs, y=y.ptr)),
            ("no plan", _launch(info, None, xs, y=y.ptr)),
            ("unaligned plan", _launch(info, plan.data_ptr() + 4, xs, y=y.ptr)),
            ("(1, 4) plan", _launch(info14, plan14, x14, y=y.ptr, sum_in=_lib.ptr(x14), sum_out=so.ptr))):
        assert rc != 0, what
        torch.cuda.synchronize()
        for b in outs + [coef]:
            b.read()
            assert b.untouched(np.zeros(b.n, dtype=bool)), what
    # ... and the handle the refusals went through still works
    assert _launch(info, plan, xs, y=y.ptr) == 0
    assert np.array_equal(_rowmajor(info, y.read()), R.case_walk(case).y0)


# ------------------------------------------------------------------------------------------ through the LightGCN handle
def _chain(words, e0, L):
    """launch_forward_lds restated: x_1 = E0, y_l = A x_l by the walk, the running sum (s + y_l) * 1 and, last, * fl(1 / (L + 1))"""
    s, x = e0, e0
    for l in range(1, L + 1):
        y = R.walk(words, x, check_banks=False).y0
        s = (s + y) * (np.float32(1.0) / np.float32(L + 1) if l == L else np.float32(1.0))
        x = y
    return s


def _handle_model(dev, form, L, fuse, e0):
    from recad_amd import model
    from tests._stub import LGN_KEYS, ReplayDataset
    case = ("edge", 16, 256, form, 0)
    U, I, rowptr, col, val = R.case_graph("edge")
    g = dict(n_users=U, n_items=I, graph_row=np.repeat(np.arange(U + I), np.diff(rowptr)), graph_col=col.astype(np.int64), graph_val=val,
             batch_len=np.zeros(0, dtype=np.int64))
    ds = ReplayDataset(g, LGN_KEYS, device=dev, steps=[])
    m = model.from_config("victim", "lightgcn", latent_dim_rec=16, lightGCN_n_layers=L, deterministic=True).I(dataset=ds)
    m.embedding_user.weight.data.copy_(torch.from_numpy(e0[:U]))
    m.embedding_item.weight.data.copy_(torch.from_numpy(e0[U:]))
    m = m.to(dev)
    m.use_lds, m.fuse_layers, m.graph_steps = True, fuse, 0
    plan, info, words = _plan(dev, case)
    graph = m._csr(m.embedding_user.weight.device)
    assert graph is m.Graph and graph.class_split == U
    graph.__dict__.setdefault("_lds", {})[16] = (plan, info)      # the forced form instead of the planner's choice
    return m, words, info


@pytest.mark.parametrize("L", [3, 5])
@pytest.mark.parametrize("form", [(2, 2), (4, 4), (2, 1), (1, 2), (4, 2), (2, 4)], ids=lambda f: f"lp{f[0]}{f[1]}")
def test_forced_forms_through_the_handle(gpu_device, form, L):
    """The staged hand-off between single launches (y_staged / x_staged) and the multi-phase launch (L = 5: 4 + 1 phases) in every
    form but the shipped one: computer() with fuse_layers off and on gives the bits of the walk chained L times; a short
    deterministic epoch (3 steps of 64 triplets) gives identical losses and tables either way; no hand-off timed out."""
    U, I = R.case_graph("edge")[:2]
    rng = np.random.default_rng(L)
    e0 = (0.1 * rng.standard_normal((U + I, 16))).astype(np.float32)
    users, pos, neg = (torch.from_numpy(rng.integers(0, hi, 3 * 64)).to(gpu_device) for hi in (U, I, I))
    outs = []
    for fuse in (False, True):
        m, words, info = _handle_model(gpu_device, form, L, fuse, e0)
        if fuse:
            R.check_multi_queues(words, 16, n_phases=4)      # only a plan whose queues cannot deadlock is launched fused
        lu, li = m.computer()
        assert m._ws["lds"][1] is info and (m._ws.get("lds_sync") is not None) == fuse
        assert (info.lpa, info.lpb) == form
        light = torch.cat([lu, li]).cpu().numpy()
        lu, li = m.computer()
        assert np.array_equal(light, torch.cat([lu, li]).cpu().numpy())
        m.check_handoffs()
        losses = m._run_epoch(users, pos, neg, 64).sum(1).cpu().numpy().copy()
        m.check_handoffs()
        assert np.isfinite(losses).all()
        outs.append((light, losses, m.embedding_user.weight.detach().cpu().numpy().copy(), m.embedding_item.weight.detach().cpu().numpy().copy()))
    want = _chain(words, e0, L)
    for k, (a, b) in enumerate(zip(*outs)):
        assert np.array_equal(a, b), ("fuse_layers off / on differ", k)
    bad = outs[0][0] != want
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4])
    assert not np.array_equal(outs[0][2], e0[:U])      # the epoch did train


def test_forms_randomised(gpu_device):
    """20 fixed-seed cases of the randomised sweep (tests/tools/spmm_lds_stress.py: random bipartite graphs, every dim % 4 == 0,
    a random form and chunk cap), compared by the same contracts; the sweep reaches forms other than the shipped one."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "spmm_lds_stress.py")
    spec = importlib.util.spec_from_file_location("spmm_lds_stress", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    forms = mod.run(seed=1234, n_cases=20, device=gpu_device)
    assert len(forms - {(1, 1)}) >= 3, sorted(forms)
