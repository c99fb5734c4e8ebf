"""GPU tests of the AushPlus kernels (recad_amd/csrc/aushplus.hip), one stage at a time: rk_ap_g_forward, rk_ap_g_backward and
rk_ap_d_step are driven through ctypes with buffers the tests own, and after a call every array the kernels left in the caller's
buffers (norm, h1, a, cls, value; zbar, bbar, eloss, dpre, all six slices of ggrad, loss; every array of D's work, dgrad, dinB,
loss) is compared, per element, with the float64 restatement of ITS stage applied to that stage's own device inputs
(tests/_aushplus_stages.py, which derives every budget by counting roundings; tests/test_aushplus_stages_host.py shows that
correct fp32 stays inside them and that ten wrong implementations do not).  Each test prints "RATIO <stage> <worst err / bound>"
before it asserts <= 1; bit-exact stages report 0 or inf.  Every output and scratch array is a view into a larger buffer of 7.0
whose guard bands must come back untouched; ggrad and dgrad start as 7.0 too, so "every element written" is tested, and the
entries / rows outside a sliced call must still hold it.

One shape, 300 items and 14 rows of 0 ... 257 entries (S.case(); test_shapes_reach_their_paths in the host file asserts what it
reaches)."""
import ctypes as C

import numpy as np
import pytest
import torch

from recad_amd import _lib

from . import _aushplus_stages as S

pytestmark = pytest.mark.gpu
EINVAL = -22
GUARD = 64
G_FLOATS = S.I * (2 * S.HG + 5) + S.HG
D_FLOATS = S.I * S.HD1 + S.HD1 + S.HD2 * S.HD1 + 2 * S.HD2 + 1
WORK_ARRAYS = (("h1", S.HD1), ("dz1", S.HD1), ("h2", S.HD2), ("dz2", S.HD2), ("p", 1), ("dlogit", 1), ("rowloss", 1))


def _report(r, prefix=""):
    for k, v in r.items():
        print(f"RATIO {prefix}{k} {v:.4f}")
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad


class Bufs:
    """named views of n floats (or int32), each GUARD floats into a buffer of n + 2 GUARD sentinels"""

    def __init__(self, dev, **sizes):
        self.whole = {k: torch.full((n + 2 * GUARD,), S.SENTINEL, device=dev) for k, n in sizes.items()}
        self.v = {k: w[GUARD:GUARD + sizes[k]] for k, w in self.whole.items()}

    def ptr(self, k):
        return C.c_void_p(self.v[k].data_ptr())

    def fetch(self):
        """the views as numpy arrays; the guard bands must hold the sentinel"""
        torch.cuda.synchronize()
        out = {}
        for k, w in self.whole.items():
            h = w.cpu().numpy()
            assert S.all_sentinel(h[:GUARD]) and S.all_sentinel(h[len(h) - GUARD:]), f"{k}: a guard band was written"
            out[k] = h[GUARD:len(h) - GUARD].copy()
        return out

    def untouched(self):
        torch.cuda.synchronize()
        return all(S.all_sentinel(w.cpu().numpy()) for w in self.whole.values())


@pytest.fixture(scope="module")
def dev_in(gpu_device):
    """the case's inputs on the device, once"""
    c = S.case()
    i32 = lambda a: torch.from_numpy(np.array(a, dtype=np.int32)).to(gpu_device)       # noqa: E731
    f32 = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).to(gpu_device)     # noqa: E731
    return {"dev": gpu_device, "rowptr": i32(c["rowptr"]), "col": i32(c["col"]), "x": f32(c["x"]), "gparam": f32(S.pack_g(c["gp"])),
            "dvalue": f32(c["dvalue"]), "rpA": i32(c["rpA"]), "colA": i32(c["colA"]), "valA": f32(c["valA"]), "i32": i32, "f32": f32}


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def _forward(d, rows):
    """rk_ap_g_forward on rows [r0, r1) of the case -> (return code, Bufs)"""
    c = S.case()
    v = S.g_view(c, rows)
    b = Bufs(d["dev"], norm=v["cap_rows"], h1=v["cap_rows"] * S.HG, a=v["E"], cls=v["E"], value=v["E"])
    rc = _lib.lib().rk_ap_g_forward(v["n"], S.I, _p(d["rowptr"], rows[0] if rows else 0), _p(d["col"]), _p(d["x"]), _p(d["gparam"]), b.ptr("norm"),
                                    b.ptr("h1"), b.ptr("a"), b.ptr("cls"), b.ptr("value"), _lib.stream_ptr(d["dev"]))
    return rc, b


def _fw_host(b):
    o = b.fetch()
    o["cls"] = o["cls"].view(np.int32)
    o["h1"] = o["h1"].reshape(-1, S.HG)
    return o


def _backward(d, rows, mode, fwb):
    """rk_ap_g_backward on the forward's device buffers -> (return code, Bufs, lists, scale)"""
    c = S.case()
    v = S.g_view(c, rows)
    lists = S.g_lists(S.I, v["rowptr"], v["col"])
    scale = S.scale_of(v) if mode == 1 else np.float32(0)
    b = Bufs(d["dev"], zbar=v["E"], bbar=4 * v["E"], eloss=v["E"], dpre=v["cap_rows"] * S.HG, ggrad=G_FLOATS, loss=1)
    tl = [d["i32"](a) for a in lists]
    e0, e1 = int(v["rowptr"][0]), int(v["rowptr"][-1])
    rc = _lib.lib().rk_ap_g_backward(v["n"], S.I, _p(d["rowptr"], rows[0] if rows else 0), _p(d["col"]), _p(d["x"]), _p(d["gparam"]), fwb.ptr("norm"),
                                     fwb.ptr("h1"), fwb.ptr("a"), mode, _p(d["dvalue"]) if mode == 0 else None, float(scale), e0, e1 - e0, _p(tl[0]),
                                     _p(tl[1]), _p(tl[2]), b.ptr("zbar"), b.ptr("bbar"), b.ptr("eloss"), b.ptr("dpre"), b.ptr("ggrad"),
                                     b.ptr("loss") if mode == 1 else None, _lib.stream_ptr(d["dev"]))
    torch.cuda.synchronize()
    return rc, b, lists, scale


def _bw_host(b):
    o = b.fetch()
    o["dpre"] = o["dpre"].reshape(-1, S.HG)
    return o


def _d_step(d, run):
    """rk_ap_d_step in one of S.D_RUNS' forms -> (return code, Bufs, sides, parameters, lists)"""
    c = S.case()
    s, dp = S.d_sides(c, run["nA"], run["nB"]), S.d_params(c, run)
    n = s["nA"] + s["nB"]
    lists = S.d_lists_of(s) if run["lists"] else None
    tl = [d["i32"](np.concatenate([a, [0]])) for a in lists] if lists else [None] * 3
    b = Bufs(d["dev"], work=n * _lib.RK_AP_D_WORK_PER_ROW, dgrad=D_FLOATS, dinB=c["E"], loss=1)
    dparam = d["f32"](S.pack_d(dp))
    A = (_p(d["rpA"], S.A_ROWS[0]), _p(d["colA"]), _p(d["valA"])) if s["nA"] else (None, None, None)
    B = (_p(d["rowptr"], S.B_ROWS[0]), _p(d["col"]), _p(d["x"])) if s["nB"] else (None, None, None)
    rc = _lib.lib().rk_ap_d_step(S.I, s["nA"], *A, run["labelA"], s["nB"], *B, run["labelB"], _p(dparam), b.ptr("work"), *(t if t is None else _p(t) for t in tl),
                                 b.ptr("dgrad") if lists else None, b.ptr("dinB") if run["din"] else None, b.ptr("loss"), _lib.stream_ptr(d["dev"]))
    torch.cuda.synchronize()
    return rc, b, s, dp, lists


def _d_host(b, n):
    o = b.fetch()
    off = 0
    for name, w in WORK_ARRAYS:
        o[name] = o["work"][off:off + n * w].reshape((n, w) if w > 1 else (n,))
        off += n * w
    assert off == len(o["work"])
    return o


def _ok(rc):
    assert rc == 0, _lib.lib().rk_last_error()


# ================================================================ 1. forward, whole and sliced
@pytest.mark.parametrize("rows", list(S.G_ROWS))
def test_forward_stages(dev_in, rows):
    c = S.case()
    rc, b = _forward(dev_in, S.G_ROWS[rows])
    _ok(rc)
    o = _fw_host(b)
    _report(S.check_g_forward(S.g_view(c, S.G_ROWS[rows]), c["gp"], o), prefix=f"fw.{rows}.")
    if rows == "whole":
        assert set(o["cls"]) == {-1, 0, 1, 2, 3, 4}, "all five classes and the boundary"
        assert np.array_equal(S.bits(o["norm"][[0, 6, 13]]), S.bits(np.full(3, 1e-12, dtype=np.float32))), "an empty row's norm is the clamp"


# ================================================================ 2. exact boundaries
def test_exact_boundaries(dev_in):
    """a == 2.5f == b_0 of item ja and == b_1 of item jb: every Heaviside pair fails, cls = -1, value = 0; backward mode 1 sees five
    zero logits there, so the entry's loss is log 5 * scale"""
    c = S.case()
    rc, fwb = _forward(dev_in, None)
    _ok(rc)
    fw = _fw_host(fwb)
    bd = S.boundaries(c["gp"]["minb"], c["gp"]["ilen"])
    assert bd[c["ja"], 0] == np.float32(2.5) and bd[c["jb"], 1] == np.float32(2.5)
    for k in (c["ka"], c["kb"]):
        assert S.bits(fw["a"][k:k + 1])[0] == S.bits(np.float32([2.5]))[0] and fw["cls"][k] == -1 and fw["value"][k] == 0 and c["x"][k] > 0
    v = S.g_view(c)
    for mode in (0, 1):
        rc, b, lists, scale = _backward(dev_in, None, mode, fwb)
        _ok(rc)
        o = _bw_host(b)
        _report(S.check_g_backward(v, c["gp"], fw, o, mode, c["dvalue"] if mode == 0 else None, scale, lists), prefix=f"boundary.bw{mode}.")
        if mode == 1:
            for k in (c["ka"], c["kb"]):
                # the eloss budget of _aushplus_stages.py at lse = log 5, dist_y = 0: scale dlse + 2 u |eloss|
                bound = float(scale) * ((S.T + 4) * S.U + (S.T + 2) * S.U * np.log(5.0))
                assert abs(float(o["eloss"][k]) - np.log(5.0) * float(scale)) <= bound


# ================================================================ 3, 4. backward, both modes, whole and sliced
@pytest.mark.parametrize("rows,mode", S.G_BACKWARD_RUNS)
def test_backward_stages(dev_in, rows, mode):
    c = S.case()
    sel = S.G_ROWS[rows]
    v = S.g_view(c, sel)
    rc, fwb = _forward(dev_in, sel)
    _ok(rc)
    fw = _fw_host(fwb)
    rc, b, lists, scale = _backward(dev_in, sel, mode, fwb)
    _ok(rc)
    o = _bw_host(b)
    _report(S.check_g_backward(v, c["gp"], fw, o, mode, c["dvalue"] if mode == 0 else None, scale, lists), prefix=f"bw{mode}.{rows}.")
    assert not np.any(S.bits(o["ggrad"]) == S.SENT_BITS), "an element of ggrad was not written"
    e0, e1 = int(v["rowptr"][0]), int(v["rowptr"][-1])
    if mode == 1:
        assert scale == np.float32(1.0 / int((c["x"][e0:e1] > 0).sum())), "scale = 1 / #(x > 0), rounded once"
        dead = np.flatnonzero(c["x"][e0:e1] <= 0) + e0
        assert len(dead) == 2 and not np.any(o["eloss"][dead]) and not np.any(o["zbar"][dead]), "entries with x <= 0 take no part"
        assert np.isfinite(o["loss"][0]) and o["loss"][0] > 0
    assert S.all_sentinel(fwb.fetch()["a"][:e0]) and fw["a"].shape == (c["E"],)


# ================================================================ 5, 6. the discriminator in every form, and saturated
@pytest.mark.parametrize("name", list(S.D_RUNS))
def test_d_step_stages(dev_in, name):
    run = S.D_RUNS[name]
    rc, b, s, dp, lists = _d_step(dev_in, run)
    _ok(rc)
    o = _d_host(b, s["nA"] + s["nB"])
    _report(S.check_d_step(s, dp, o, run["labelA"], run["labelB"], lists, run["din"]), prefix=f"d.{name}.")
    if lists:
        assert not np.any(S.bits(o["dgrad"]) == S.SENT_BITS), "an element of dgrad was not written"
    if run["b3"] is not None:
        assert np.all(o["p"] == (1.0 if run["b3"] > 0 else 0.0)) and np.all(np.isfinite(o["dgrad"])) and np.all(o["dlogit"] == 0)
        lab = np.array([run["labelA"]] * s["nA"] + [run["labelB"]] * s["nB"])
        side = np.array([s["nA"]] * s["nA"] + [s["nB"]] * s["nB"])
        assert np.array_equal(o["rowloss"] != 0, lab != o["p"]) and np.allclose(o["rowloss"][lab != o["p"]], (100.0 / side)[lab != o["p"]], rtol=4 * S.U)


# ================================================================ 7. twice to the same bits
def test_two_runs_give_the_same_bits(dev_in):
    def once():
        out = {}
        for rows, mode in S.G_BACKWARD_RUNS:
            rc, fwb = _forward(dev_in, S.G_ROWS[rows])
            _ok(rc)
            rc, b, _, _ = _backward(dev_in, S.G_ROWS[rows], mode, fwb)
            _ok(rc)
            out.update({f"fw.{rows}.{mode}.{k}": a for k, a in fwb.fetch().items()})
            out.update({f"bw.{rows}.{mode}.{k}": a for k, a in b.fetch().items()})
        for name in ("full", "adversarial", "nB0", "no_dgrad", "no_din"):
            rc, b, _, _, _ = _d_step(dev_in, S.D_RUNS[name])
            _ok(rc)
            out.update({f"d.{name}.{k}": a for k, a in b.fetch().items()})
        return out

    first, second = once(), once()
    diff = [k for k in first if not np.array_equal(S.bits(first[k]), S.bits(second[k]))]
    assert not diff, diff


# ================================================================ 8. refusals
def _refused(fn, args, bufs, what):
    assert fn(*args) == EINVAL, what
    assert bufs.untouched(), f"{what}: refused, but a buffer was written"


def test_forward_refusals(dev_in):
    d, c = dev_in, S.case()
    b = Bufs(d["dev"], norm=c["n_rows"], h1=c["n_rows"] * S.HG, a=c["E"], cls=c["E"], value=c["E"])
    base = [c["n_rows"], S.I, _p(d["rowptr"]), _p(d["col"]), _p(d["x"]), _p(d["gparam"]), b.ptr("norm"), b.ptr("h1"), b.ptr("a"), b.ptr("cls"),
            b.ptr("value"), _lib.stream_ptr(d["dev"])]
    fn = _lib.lib().rk_ap_g_forward
    for i in range(2, 11):
        _refused(fn, base[:i] + [None] + base[i + 1:], b, f"argument {i} NULL")
    for i, val in ((0, -1), (1, 0), (1, -1)):
        _refused(fn, base[:i] + [val] + base[i + 1:], b, f"argument {i} = {val}")
    assert fn(*([0] + base[1:])) == 0 and fn(0, S.I, *([None] * 9), base[11]) == 0, "n_rows = 0 is an empty call, not an error"
    assert b.untouched()


def test_backward_refusals(dev_in):
    d, c = dev_in, S.case()
    lists = [d["i32"](a) for a in S.g_lists(S.I, c["rowptr"], c["col"])]
    b = Bufs(d["dev"], norm=c["n_rows"], h1=c["n_rows"] * S.HG, a=c["E"], zbar=c["E"], bbar=4 * c["E"], eloss=c["E"], dpre=c["n_rows"] * S.HG,
             ggrad=G_FLOATS, loss=1)
    base = [c["n_rows"], S.I, _p(d["rowptr"]), _p(d["col"]), _p(d["x"]), _p(d["gparam"]), b.ptr("norm"), b.ptr("h1"), b.ptr("a"), 0, _p(d["dvalue"]), 1.0,
            0, c["E"], _p(lists[0]), _p(lists[1]), _p(lists[2]), b.ptr("zbar"), b.ptr("bbar"), b.ptr("eloss"), b.ptr("dpre"), b.ptr("ggrad"), b.ptr("loss"),
            _lib.stream_ptr(d["dev"])]
    fn = _lib.lib().rk_ap_g_backward
    sub = lambda i, val, a=base: a[:i] + [val] + a[i + 1:]                  # noqa: E731
    for i in list(range(2, 9)) + list(range(14, 22)):
        for mode in (0, 1):
            _refused(fn, sub(i, None, sub(9, mode)), b, f"mode {mode}, argument {i} NULL")
    _refused(fn, sub(10, None), b, "mode 0 without dvalue")
    _refused(fn, sub(22, None, sub(9, 1)), b, "mode 1 without loss")
    for i, val in ((9, 2), (9, -1), (0, 0), (0, -1), (1, 0), (1, -1), (12, -1), (13, -1)):
        _refused(fn, sub(i, val), b, f"argument {i} = {val}")


def test_d_step_refusals(dev_in):
    d, c = dev_in, S.case()
    s = S.d_sides(c)
    lists = [d["i32"](np.concatenate([a, [0]])) for a in S.d_lists_of(s)]
    b = Bufs(d["dev"], work=(S.NA + S.NB) * _lib.RK_AP_D_WORK_PER_ROW, dgrad=D_FLOATS, dinB=c["E"], loss=1)
    dparam = d["f32"](S.pack_d(c["dp"]))
    base = [S.I, S.NA, _p(d["rpA"], S.A_ROWS[0]), _p(d["colA"]), _p(d["valA"]), 1.0, S.NB, _p(d["rowptr"], S.B_ROWS[0]), _p(d["col"]), _p(d["x"]), 0.0,
            _p(dparam), b.ptr("work"), _p(lists[0]), _p(lists[1]), _p(lists[2]), b.ptr("dgrad"), b.ptr("dinB"), b.ptr("loss"), _lib.stream_ptr(d["dev"])]
    fn = _lib.lib().rk_ap_d_step
    sub = lambda i, val, a=base: a[:i] + [val] + a[i + 1:]                  # noqa: E731
    for i in (2, 3, 4, 7, 8, 9, 11, 12, 18):
        _refused(fn, sub(i, None), b, f"argument {i} NULL")
    for i in (13, 14, 15):
        _refused(fn, sub(i, None), b, f"dgrad without list {i}")
    for i, val in ((0, 0), (0, -1), (1, -1), (6, -1)):
        _refused(fn, sub(i, val), b, f"argument {i} = {val}")
    _refused(fn, sub(1, 0, sub(6, 0)), b, "nA + nB == 0")
    _refused(fn, sub(1, 1, sub(6, -1)), b, "nA + nB > 0 with nB < 0")
