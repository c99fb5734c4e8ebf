"""GPU tests of csrc/pga.hip one entry point at a time, on the case table of tests/_pga_restate.py.  The chain is run once per case
and repetition on the device, every entry's inputs being the device's own upstream outputs and every output sitting behind
sentinel guards; each test then holds one entry's output to the restatement of that stage from the same device inputs.

Exact: D's zeros, the selection and the new CSR, the pinning, max|grad| given grad, the update given grad, rk_ials_solve_rhs with
rhs = b_u against rk_ials_half_sweep, and every entry run twice.  Z and V follow rk_ials_half_sweep's rule on a sample of rows (the
empty, the shortest and the longest among them): 4 x the fp32 walk's error on the system rk_ials_system wrote + 2^-23 max|x*|, and
the hard bound.  The loss, D, g, M, h and grad sit inside their budgets (tests/_pga_restate.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from recad_amd import _lib
from tests import _ials_restate as IR
from tests import _pga_restate as P
from tests._gemm_forms import Guarded

pytestmark = pytest.mark.gpu
IDS = [P.case_id(c) for c in P.CASES]
BLOCK = 64                       # users per block of the loss: U = 70 and 300 put a block boundary inside it
LR = 0.25
EINVAL = -22
DSENT = 2.0 ** -300


def _t(a, dev, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _gemm(M, N, K, a, a_rs, a_cs, b, b_rs, b_cs, c, ldc):
    g = _lib.GemmDesc()
    g.M, g.N, g.K, g.policy = M, N, K, 0
    g.A, g.a_rs, g.a_cs, g.B, g.b_rs, g.b_cs, g.C, g.ldc = a, a_rs, a_cs, b, b_rs, b_cs, c, ldc
    _lib.check(_lib.lib().rk_gemm_f32(C.byref(g), None, None, _lib.stream_ptr()), "rk_gemm_f32")


def _vp(addr):
    return C.c_void_p(addr)


@functools.lru_cache(maxsize=None)
def _run(c, rep):
    """The whole chain of one case on the device -> every stage's output as numpy (rep only keys the cache: the second run)."""
    dev = torch.device("cuda:0")
    k = P.case(c)
    d, I, U, A, F, tg = k["d"], k["I"], k["U"], k["A"], k["F"], k["targets"]
    alpha, lam, w = k["alpha"], k["lam"], float(k["wbar"])
    L, p, s = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    ok = lambda rc, what: _lib.check(rc, what)   # noqa: E731
    n_rows, ln = U + A, len(tg) + F
    cp, ci, cv = P.combined_csr(k["ptr"], k["idx"], k["val"], k["cols"], P.RATING)
    rowptr, col, val = _t(cp, dev, np.int32), _t(ci, dev, np.int32), _t(cv, dev, np.float32)
    nnz = len(ci)
    colptr = torch.empty(I + 1, dtype=torch.int32, device=dev)
    crow, cval = torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.float32, device=dev)
    ok(L.rk_pca_transpose(n_rows, I, p(rowptr), p(col), p(val), p(colptr), p(crow), p(cval), s), "rk_pca_transpose")
    fptr = _t(np.arange(A + 1) * ln, dev, np.int32)
    fcol, fval = col[len(k["idx"]):], val[len(k["idx"]):]
    Yo = _t(k["Yo"], dev, np.float32)
    dp = (d + 15) // 16 * 16
    work = torch.empty(((max(n_rows, I) + 255) // 256) * dp * dp, dtype=torch.float32, device=dev)
    Go, Gx = torch.empty(d * d, dtype=torch.float32, device=dev), torch.empty(d * d, dtype=torch.float32, device=dev)
    status = torch.zeros(8, dtype=torch.int32, device=dev)
    X, Yp = Guarded(dev, n_rows * d), Guarded(dev, I * d)
    ok(L.rk_ials_gram(I, d, p(Yo), lam, p(Go), p(work), work.numel(), s), "gram")
    ok(L.rk_ials_half_sweep(n_rows, I, d, p(Go), p(rowptr), p(col), p(val), alpha, p(Yo), None, _vp(X.ptr), p(status[0:2]), s), "half")
    ok(L.rk_ials_gram(n_rows, d, _vp(X.ptr), lam, p(Gx), p(work), work.numel(), s), "gram")
    ok(L.rk_ials_half_sweep(I, n_rows, d, p(Gx), p(colptr), p(crow), p(cval), alpha, _vp(X.ptr), None, _vp(Yp.ptr), p(status[2:4]), s), "half")
    out = {"X": X.read().reshape(n_rows, d).copy(), "Yp": Yp.read().reshape(I, d).copy(), "guards": [X.untouched(), Yp.untouched()]}
    # rk_ials_solve_rhs with rhs = b_u against the half-sweep, over the user side
    ids = torch.arange(n_rows, dtype=torch.int32, device=dev)
    A_sys, b_sys = torch.empty(n_rows * d * d, dtype=torch.float32, device=dev), torch.empty(n_rows * d, dtype=torch.float32, device=dev)
    ok(L.rk_ials_system(I, d, p(Go), p(rowptr), p(col), p(val), alpha, p(Yo), n_rows, p(ids), p(A_sys), p(b_sys), s), "system")
    Xb = Guarded(dev, n_rows * d)
    ok(L.rk_ials_solve_rhs(n_rows, I, d, p(Go), p(rowptr), p(col), p(val), alpha, p(Yo), p(b_sys), None, _vp(Xb.ptr), p(status[4:6]), s), "rhs")
    out["X_from_b"] = Xb.read().reshape(n_rows, d).copy()
    out["guards"].append(Xb.untouched())
    # the loss: per target and block the scores, D and the block's part of g
    rp, rc_ = rowptr, col                            # the real rows lead the combined CSR (and its arrays are never empty)
    blocks = [(u0, min(BLOCK, U - u0)) for u0 in range(0, U, BLOCK)]
    n_parts = len(tg) * len(blocks)
    parts = Guarded(dev, n_parts * I * d)
    terms = torch.full((len(tg) * U + 2,), DSENT, dtype=torch.float64, device=dev)
    out["S"], out["D"], out["elig"], at = [], [], [], 0
    for ti, t in enumerate(tg):
        e = P.eligible(k["ptr"], k["idx"], U, t)
        el = _t(e, dev, np.int32)
        out["elig"].append(e)
        for u0, nb in blocks:
            S = Guarded(dev, nb * I)
            xb = X.ptr + 4 * u0 * d
            _gemm(nb, I, d, xb, d, 1, Yp.ptr, d, 1, S.ptr, I)
            out["S"].append(S.read().reshape(nb, I).copy())
            ok(L.rk_pga_loss(nb, I, _vp(S.ptr), p(rp), p(rc_), u0, t, p(el), 1.0 / e.sum(), _vp(terms.data_ptr() + 8 * (1 + ti * U + u0)), s),
               "rk_pga_loss")
            out["D"].append(S.read().reshape(nb, I).copy())
            out["guards"].append(S.untouched())
            _gemm(I, d, nb, S.ptr, 1, I, xb, 1, d, parts.ptr + 4 * at * I * d, d)
            at += 1
    g = Guarded(dev, I * d)
    loss = torch.full((3,), DSENT, dtype=torch.float64, device=dev)
    ok(L.rk_pga_add_blocks(I * d, n_parts, _vp(parts.ptr), _vp(g.ptr), s), "rk_pga_add_blocks")
    ok(L.rk_pga_loss_sum(len(tg) * U, _vp(terms.data_ptr() + 8), _vp(loss.data_ptr() + 8), s), "rk_pga_loss_sum")
    out["parts"] = parts.read().reshape(n_parts, I, d).copy()
    out["g"], out["terms"], out["loss"] = g.read().reshape(I, d).copy(), terms.cpu().numpy(), loss.cpu().numpy()
    out["guards"] += [parts.untouched(), g.untouched()]
    Z, M, H, V, grad = Guarded(dev, I * d), Guarded(dev, d * d), Guarded(dev, A * d), Guarded(dev, A * d), Guarded(dev, A * I)
    gmax = torch.full((3,), 0x7FFFFFFF, dtype=torch.int32, device=dev)
    xf = X.ptr + 4 * U * d
    ok(L.rk_ials_solve_rhs(I, n_rows, d, p(Gx), p(colptr), p(crow), p(cval), alpha, _vp(X.ptr), _vp(g.ptr), None, _vp(Z.ptr), p(status[4:6]), s), "Z")
    _gemm(d, d, I, Z.ptr, 1, d, Yp.ptr, 1, d, M.ptr, d)
    ok(L.rk_pga_user_adjoint(A, I, d, _vp(Z.ptr), _vp(Yp.ptr), _vp(xf), _vp(M.ptr), p(fptr), p(fcol), w, _vp(H.ptr), s), "adjoint")
    ok(L.rk_ials_solve_rhs(A, I, d, p(Go), p(fptr), p(fcol), p(fval), alpha, p(Yo), _vp(H.ptr), None, _vp(V.ptr), p(status[6:8]), s), "V")
    ok(L.rk_pga_grad(A, I, d, _vp(xf), _vp(V.ptr), _vp(Z.ptr), _vp(Yp.ptr), p(Yo), w, _vp(grad.ptr), _vp(gmax.data_ptr() + 4), s), "grad")
    for name, buf, shape in (("Z", Z, (I, d)), ("M", M, (d, d)), ("H", H, (A, d)), ("V", V, (A, d)), ("grad", grad, (A, I))):
        out[name] = buf.read().reshape(shape).copy()
        out["guards"].append(buf.untouched())
    out["gmax"] = gmax.cpu().numpy().view(np.uint32)
    # the systems of a sample of rows, as the device built them
    for side, n, G_, csr, Y_ in (("z", I, Gx, (colptr, crow, cval), X.ptr), ("v", A, Go, (fptr, fcol, fval), Yo.data_ptr())):
        lens = np.diff(csr[0].cpu().numpy())
        order = np.argsort(lens, kind="stable")
        rows = np.unique(np.r_[order[:3], order[-3:], np.random.default_rng(k["rng_seed"]).choice(n, size=min(n, 8), replace=False)])
        rid = _t(rows, dev, np.int32)
        As, bs = torch.empty(len(rows) * d * d, dtype=torch.float32, device=dev), torch.empty(len(rows) * d, dtype=torch.float32, device=dev)
        ok(L.rk_ials_system(I if side == "v" else n_rows, d, p(G_), p(csr[0]), p(csr[1]), p(csr[2]), alpha, _vp(Y_), len(rows), p(rid),
                            p(As), p(bs), s), "system")
        out["sys_" + side] = (rows, As.cpu().numpy().reshape(len(rows), d, d))
    # the step, from strengths with many ties, and the selection alone
    rng = np.random.default_rng(k["rng_seed"] + 1)
    R_in = (np.round(rng.random((A, I)) * 8) / 8).astype(np.float32)
    tgt = _t(tg, dev, np.int32)
    for name, with_grad in (("step", True), ("select", False)):
        R = Guarded(dev, A * I, fill=R_in.reshape(-1))
        fc = torch.full((A * ln + 2,), -7, dtype=torch.int32, device=dev)
        ok(L.rk_pga_step(A, I, _vp(R.ptr), _vp(grad.ptr) if with_grad else None, _vp(gmax.data_ptr() + 4) if with_grad else None, LR, len(tg),
                         p(tgt), F, _vp(fc.data_ptr() + 4), s), "rk_pga_step")
        out[name] = (R.read().reshape(A, I).copy(), fc.cpu().numpy())
        out["guards"].append(R.untouched())
    out["R_in"], out["status"] = R_in, status.cpu().numpy()
    torch.cuda.synchronize()
    return out


def _csc(k):
    cp, ci, cv = P.combined_csr(k["ptr"], k["idx"], k["val"], k["cols"], P.RATING)
    return IR.transpose(cp, ci, cv, k["I"])


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_guards_status_and_solve_rhs_equals_half_sweep(gpu_device, c):
    o = _run(c, 0)
    assert all(o["guards"]), "an entry wrote outside its output"
    assert o["status"].tolist() == [0, -1] * 4
    assert np.array_equal(o["X_from_b"].view(np.uint32), o["X"].view(np.uint32)), "rhs = b_u reproduces rk_ials_half_sweep bit for bit"
    assert o["gmax"][0] == 0x7FFFFFFF and o["gmax"][2] == 0x7FFFFFFF


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_loss_terms_and_d(gpu_device, c):
    k, o = P.case(c), _run(c, 0)
    U, I = k["U"], k["I"]
    blocks = [(u0, min(BLOCK, U - u0)) for u0 in range(0, U, BLOCK)]
    terms = o["terms"]
    assert terms[0] == DSENT and terms[-1] == DSENT and o["loss"][0] == DSENT and o["loss"][2] == DSENT
    at, total, total_abs = 0, 0.0, 0.0
    for ti, t in enumerate(k["targets"]):
        e = o["elig"][ti]
        inv = 1.0 / e.sum()
        for u0, nb in blocks:
            S, D = o["S"][at], o["D"][at]
            D64, t64 = P.loss_stage64(S, k["ptr"], k["idx"], u0, t, e, inv)
            got_t = terms[1 + ti * U + u0: 1 + ti * U + u0 + nb]
            assert np.all(np.abs(D.astype(np.float64) - D64) <= P.d_budget(D64, inv)), (t, u0)
            assert np.all(np.abs(got_t - t64) <= P.term_budget(S, t, t64, inv)), (t, u0)
            zero = np.zeros((nb, I), dtype=bool)                 # rated items, and the rows of users outside E_t: exactly +0.0f
            for b in range(nb):
                u = u0 + b
                zero[b, k["idx"][k["ptr"][u]:k["ptr"][u + 1]]] = True
                if not e[u]:
                    zero[b] = True
                    assert got_t[b] == 0.0
            assert not D.view(np.uint32)[zero].any()
            if e[u0:u0 + nb].any():
                assert np.all(D[e[u0:u0 + nb], t] <= 0)          # 0 for the user whose only unrated item is the target
            total += got_t.sum()
            total_abs += np.abs(got_t).sum()
            at += 1
    assert abs(o["loss"][1] - total) <= (len(terms) + 8) * 2.0 ** -53 * total_abs


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_g_and_m(gpu_device, c):
    k, o = P.case(c), _run(c, 0)
    U = k["U"]
    blocks = [(u0, min(BLOCK, U - u0)) for u0 in range(0, U, BLOCK)] * len(k["targets"])
    Xs = [o["X"][u0:u0 + nb] for u0, nb in blocks]
    assert np.all(np.abs(o["g"].astype(np.float64) - P.g_stage64(o["D"], Xs)) <= P.g_budget(o["D"], Xs))
    walk = o["parts"][0].copy()
    for part in o["parts"][1:]:
        walk = walk + part
    assert np.array_equal(walk.view(np.uint32), o["g"].view(np.uint32)), "the parts added in order"
    assert np.all(np.abs(o["M"].astype(np.float64) - P.m_stage64(o["Z"], o["Yp"])) <= P.m_budget(o["Z"], o["Yp"]))


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_z_and_v_follow_the_half_sweep_rule(gpu_device, c):
    k, o = P.case(c), _run(c, 0)
    U = k["U"]
    for side, got, rhs, (ptr, idx, val), Y, n in (("z", o["Z"], o["g"], _csc(k), o["X"], U + k["A"]),
                                                  ("v", o["V"], o["H"], P.fake_csr(k["cols"], P.RATING), k["Yo"], k["I"])):
        G64 = IR.gram64(Y, k["lam"])
        rows, As = o["sys_" + side]
        for r, A_dev in zip(rows, As):
            sl = slice(ptr[r], ptr[r + 1])
            A64, _ = IR.system64(G64, Y, idx[sl], val[sl], k["alpha"])
            x = IR.solve64(A64, rhs[r].astype(np.float64))
            xw = IR.solve_walk(A_dev, rhs[r])
            assert xw is not None
            walk_err = float(np.abs(xw.astype(np.float64) - x).max())
            err = float(np.abs(got[r].astype(np.float64) - x).max())
            kappa, hard = P.hard_rhs(A64, x, ptr[r + 1] - ptr[r], n)
            assert kappa <= P.KAPPA_CAP * 1.01 and err <= IR.x_budget(walk_err, x) and err <= hard, (side, r, err, walk_err, hard, kappa)


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_h_and_grad(gpu_device, c):
    k, o = P.case(c), _run(c, 0)
    U, w = k["U"], k["wbar"]
    Xf = o["X"][U:]
    H64 = P.h_stage64(o["Z"], o["Yp"], Xf, o["M"], k["cols"], w)
    assert np.all(np.abs(o["H"].astype(np.float64) - H64) <= P.h_budget(o["Z"], o["Yp"], Xf, o["M"], k["cols"], w))
    g64 = P.grad_stage64(Xf, o["V"], o["Z"], o["Yp"], k["Yo"], w)
    assert np.all(np.abs(o["grad"].astype(np.float64) - g64) <= P.grad_budget(Xf, o["V"], o["Z"], o["Yp"], k["Yo"], w))
    assert o["gmax"][1] == P.max_abs_bits(o["grad"]), "max|grad| given grad, exactly"


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_step_update_pinning_and_selection_are_exact(gpu_device, c):
    k, o = P.case(c), _run(c, 0)
    tg, F, ln = k["targets"], k["F"], len(k["targets"]) + k["F"]
    for name, bits in (("step", int(o["gmax"][1])), ("select", 0)):
        R_out, fc = o[name]
        want = P.update_walk(o["R_in"], o["grad"], bits, LR, tg)
        assert np.array_equal(R_out.view(np.uint32), want.view(np.uint32)), name
        assert np.all(R_out[:, tg] == 1.0) and R_out.min() >= 0.0 and R_out.max() <= 1.0
        assert fc[0] == -7 and fc[-1] == -7
        assert np.array_equal(fc[1:-1].reshape(k["A"], ln), P.select(R_out, tg, F)), name
    if o["gmax"][1] == 0:
        assert np.array_equal(o["step"][0], o["select"][0]), "an all-zero gradient leaves R alone"


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_two_runs_give_the_same_bits(gpu_device, c):
    a, b = _run(c, 0), _run(c, 1)
    for name in ("X", "Yp", "g", "Z", "M", "H", "V", "grad", "terms", "loss", "gmax", "parts"):
        assert np.array_equal(np.ascontiguousarray(a[name]).view(np.uint8), np.ascontiguousarray(b[name]).view(np.uint8)), name
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a["D"], b["D"]))
    for name in ("step", "select"):
        assert np.array_equal(a[name][0].view(np.uint32), b[name][0].view(np.uint32)) and np.array_equal(a[name][1], b[name][1])


def test_the_transpose_the_chain_relies_on(gpu_device):
    """rk_pca_transpose of the combined CSR: users ascending inside an item's row, which fixes the order of every item-side sum."""
    k = P.case(P.CASES[4])
    cp, ci, cv = P.combined_csr(k["ptr"], k["idx"], k["val"], k["cols"], P.RATING)
    L, p, s = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    dev = gpu_device
    colptr = torch.empty(k["I"] + 1, dtype=torch.int32, device=dev)
    crow, cval = torch.empty(len(ci), dtype=torch.int32, device=dev), torch.empty(len(ci), dtype=torch.float32, device=dev)
    rowptr, col, val = _t(cp, dev, np.int32), _t(ci, dev, np.int32), _t(cv, dev, np.float32)      # named: they outlive the call
    _lib.check(L.rk_pca_transpose(k["U"] + k["A"], k["I"], p(rowptr), p(col), p(val), p(colptr), p(crow), p(cval), s), "rk_pca_transpose")
    tp = IR.transpose(cp, ci, cv, k["I"])
    assert np.array_equal(colptr.cpu().numpy(), tp[0]) and np.array_equal(crow.cpu().numpy(), tp[1]) and np.array_equal(cval.cpu().numpy(), tp[2])


def test_solve_rhs_reports_the_lowest_row_it_cannot_factorise(gpu_device):
    """5 rows x 4 items, d = 2.  A NaN in item 2's factors reaches the systems of rows 1 and 3 only: the lower one is reported, in
    either order of the rows; the clean table leaves (0, -1).  A refusal here is in the status words, the call returns 0."""
    dev = gpu_device
    L, p, s = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    rows = [[0, 1], [1, 2], [0, 3], [2, 3], [0]]
    rowptr = _t(np.r_[0, np.cumsum([len(r) for r in rows])], dev, np.int32)
    col, val = _t(np.concatenate(rows), dev, np.int32), _t(np.ones(9), dev, np.float32)
    Y = (np.arange(8, dtype=np.float32).reshape(4, 2) + 1) / 8
    G, rhs = _t(np.eye(2), dev, np.float32), _t(np.ones((5, 2)), dev, np.float32)
    status = torch.full((4,), -7, dtype=torch.int32, device=dev)
    for nan_at, order, want in ((None, None, [0, -1]), ((2, 1), None, [_lib.RK_IALS_NOT_SPD, 1]), ((2, 0), [4, 3, 2, 1, 0], [_lib.RK_IALS_NOT_SPD, 1])):
        Yd = Y.copy()
        if nan_at:
            Yd[nan_at] = np.nan
        Yt, od = _t(Yd, dev, np.float32), (None if order is None else _t(order, dev, np.int32))
        X = Guarded(dev, 5 * 2)
        rc = L.rk_ials_solve_rhs(5, 4, 2, p(G), p(rowptr), p(col), p(val), 1.0, p(Yt), p(rhs), p(od), _vp(X.ptr), p(status[1:3]), s)
        torch.cuda.synchronize()
        assert rc == 0 and status.cpu().tolist() == [-7] + want + [-7], (nan_at, order)
        x = X.read().reshape(5, 2)
        solved = np.array([nan_at is None or 2 not in r for r in rows])
        assert X.untouched(np.repeat(solved, 2)) and np.all(np.isfinite(x[solved])), "a refused row is left as it was"


def test_every_refusal_writes_nothing(gpu_device):
    dev = gpu_device
    L, p, s = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    buf = Guarded(dev, 4096)
    ints = torch.full((64,), -7, dtype=torch.int32, device=dev)
    dbl = torch.full((8,), DSENT, dtype=torch.float64, device=dev)
    rowptr, col = _t([0, 1, 2], dev, np.int32), _t([0, 1], dev, np.int32)
    val = _t([1, 1], dev, np.float32)
    B, Pi, Pd = _vp(buf.ptr), p(ints), p(dbl)
    nan, inf = float("nan"), float("inf")
    calls = [
        L.rk_ials_solve_rhs(0, 2, 2, B, p(rowptr), p(col), p(val), 1.0, B, B, None, B, Pi, s),
        L.rk_ials_solve_rhs(2, 0, 2, B, p(rowptr), p(col), p(val), 1.0, B, B, None, B, Pi, s),
        L.rk_ials_solve_rhs(2, 2, 0, B, p(rowptr), p(col), p(val), 1.0, B, B, None, B, Pi, s),
        L.rk_ials_solve_rhs(2, 2, 129, B, p(rowptr), p(col), p(val), 1.0, B, B, None, B, Pi, s),
        L.rk_ials_solve_rhs(2, 2, 2, B, p(rowptr), p(col), p(val), -1.0, B, B, None, B, Pi, s),
        L.rk_ials_solve_rhs(2, 2, 2, B, p(rowptr), p(col), p(val), nan, B, B, None, B, Pi, s),
        L.rk_ials_solve_rhs(2, 2, 2, B, p(rowptr), p(col), p(val), 1.0, B, None, None, B, Pi, s),
        L.rk_ials_solve_rhs(2, 2, 2, B, p(rowptr), p(col), p(val), 1.0, B, B, None, B, None, s),
        L.rk_pga_loss(0, 2, B, p(rowptr), p(col), 0, 0, Pi, 1.0, Pd, s),
        L.rk_pga_loss(2, 2, B, p(rowptr), p(col), -1, 0, Pi, 1.0, Pd, s),
        L.rk_pga_loss(2, 2, B, p(rowptr), p(col), 0, 2, Pi, 1.0, Pd, s),
        L.rk_pga_loss(2, 2, B, p(rowptr), p(col), 0, -1, Pi, 1.0, Pd, s),
        L.rk_pga_loss(2, 2, B, p(rowptr), p(col), 0, 0, Pi, 0.0, Pd, s),
        L.rk_pga_loss(2, 2, B, p(rowptr), p(col), 0, 0, Pi, inf, Pd, s),
        L.rk_pga_loss(2, 2, B, p(rowptr), p(col), 0, 0, None, 1.0, Pd, s),
        L.rk_pga_loss_sum(0, Pd, Pd, s), L.rk_pga_loss_sum(2, None, Pd, s),
        L.rk_pga_add_blocks(0, 1, B, B, s), L.rk_pga_add_blocks(4, 0, B, B, s), L.rk_pga_add_blocks(4, 1, B, None, s),
        L.rk_pga_user_adjoint(0, 2, 2, B, B, B, B, p(rowptr), p(col), 1.0, B, s),
        L.rk_pga_user_adjoint(2, 2, 129, B, B, B, B, p(rowptr), p(col), 1.0, B, s),
        L.rk_pga_user_adjoint(2, 2, 2, B, B, B, B, p(rowptr), p(col), nan, B, s),
        L.rk_pga_user_adjoint(2, 2, 2, B, B, B, None, p(rowptr), p(col), 1.0, B, s),
        L.rk_pga_grad(0, 2, 2, B, B, B, B, B, 1.0, B, Pi, s), L.rk_pga_grad(2, 0, 2, B, B, B, B, B, 1.0, B, Pi, s),
        L.rk_pga_grad(2, 2, 0, B, B, B, B, B, 1.0, B, Pi, s), L.rk_pga_grad(2, 2, 2, B, B, B, B, B, -1.0, B, Pi, s),
        L.rk_pga_grad(2, 2, 2, B, B, B, B, B, 1.0, B, None, s),
        L.rk_pga_step(0, 4, B, B, Pi, 0.25, 1, p(col), 1, Pi, s), L.rk_pga_step(2, 4, B, B, Pi, 0.25, 0, p(col), 1, Pi, s),
        L.rk_pga_step(2, 4, B, B, Pi, 0.25, 65, p(col), 1, Pi, s), L.rk_pga_step(2, 4, B, B, Pi, 0.25, 1, p(col), 4, Pi, s),
        L.rk_pga_step(2, 4, B, B, Pi, 0.25, 1, p(col), -1, Pi, s), L.rk_pga_step(2, 4, B, B, Pi, 0.0, 1, p(col), 1, Pi, s),
        L.rk_pga_step(2, 4, B, B, Pi, nan, 1, p(col), 1, Pi, s), L.rk_pga_step(2, 4, B, B, None, 0.25, 1, p(col), 1, Pi, s),
        L.rk_pga_step(2, 4, B, None, None, 0.25, 1, None, 1, Pi, s),
    ]
    torch.cuda.synchronize()
    assert calls == [EINVAL] * len(calls), calls
    buf.read()
    assert buf.untouched(np.zeros(4096, dtype=bool)) and ints.cpu().tolist() == [-7] * 64 and dbl.cpu().tolist() == [DSENT] * 8
    assert b"rk_pga_step" in _lib.lib().rk_last_error()
