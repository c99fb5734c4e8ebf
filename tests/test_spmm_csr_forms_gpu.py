"""Every form of the row-gather SpMM (recad_amd/csrc/spmm.h) on the device, bit for bit against the walk of its own schedule
(tests/_spmm_restate.py).  The shipped builder only ever picks 4 waves per workgroup below 8 M nonzeros, segments of 128 only when
half the nonzeros sit in long rows, and packing only when a quarter of the rows is short; the schedules here are built by
rk_csr_schedule_build_host_ex, uploaded by rk_csr_schedule_upload and launched through rk_spmm_csr_ex / rk_spmm_csr (and, seeded
into a CsrGraph's schedule cache, through the LightGCN handle: graph dropout, the marked block list).  The same cases pass
tests/test_spmm_csr_forms_host.py on the CPU first: structure, the rounding budget against float64, and that the cases tell a
wrong summation order from the right one.

Case graph, one per (dim, W, seg), ~300 rows, x taller than the graph (as many rows as the longest row has columns; dim 256 at
W = 16, seg = 128: 18 437 rows of x).  With G = dim / 4: two empty rows, a row of 1; G - 1, G, G + 1 (the packing boundary);
seg - 1, seg, seg + 1, 2 seg + 1, W seg (fills a workgroup); W seg + 1 (two pieces, the second of ONE entry); 8 W seg + 1 (9 pieces:
one unrolled round of piece_arrive's slot reads); 9 W seg + 5 (10 pieces: a round and a tail); a Poisson body on both sides of G.
Values and x are normal fp32, no subnormals.

Forms: dims 32 / 64 / 128 / 256 x W 4 / 8 / 16 x seg 64 / 128 without packing; packing forced on at 32 / 64 / 128; dims 48 / 100 / 7 on
the generic kernel x W 4 / 8 / 16; class_split in the middle on a subset.

Contracts (u = 2^-24):
  y, no addend   np.array_equal with the walk
  addend         v == fl(walk + add): one fp32 add
  running sum    sum_out == fl(fl(sum_in + v) * scale), v the kernel's own y when y is requested, else the walk through the addend
                 contract ((a + b) * c is an add then a multiply: nothing to fuse)
  zero1 / zero2  exact zeros on every row of the slab; what is not requested keeps its sentinel
  Adam           adam_t > 0, and adam_t < 0 behind rk_adam_coef_advance: p / m / v == orc.adam on the kernel's own v
  src_filter     bit-equal to the filtered walk at ~3 % and ~50 %, a bitmap that hits all 64 lanes of one chunk, one hit, none;
                 all ones gives the bits of the unfiltered walk, all zeros gives add or 0; add == x with the filter on every form
Every output sits behind sentinel guards; every launch is repeated and must repeat bit for bit (the long rows' arrival counters
reset themselves: one scratch block per form serves every launch of this file and its counters are zero in the end).

X must be finite (include/recad_hip.h): a padding lane gathers x[0] and multiplies it by zero.  The test here asserts what the
header promises: a non-finite row of x that is neither row 0 nor referenced leaves every output finite.

Out of scope: the slot area beyond a buffer descriptor's 2 GiB (slot_bytes > 0x7fffffff) cannot be reached at small shapes; the
RK_TUNING variants; the automatic choice of 8 waves above 8 M nonzeros stays with the full-size tests; the backward's tpos path
keeps its oracle test (tests/test_gpu_parity.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from recad_amd import _lib
from tests import _drop_restate as DR
from tests import _spmm_restate as R
from tests._gemm_forms import SENT, Guarded

pytestmark = pytest.mark.gpu

_sched, _graphs, _xs = {}, {}, {}


def _t(dev, a):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)


def _upload(dev, rowptr, split, dim, form):
    """-> (wave_desc device tensor, n_blocks, scratch (zero-filled, or None), words)"""
    rc, h, nb, nw, sw = R.build_handle(rowptr, split, dim, form)
    assert rc == 0, _lib.lib().rk_last_error()
    try:
        words = R.handle_words(h, nw)
        desc = torch.zeros(nw, device=dev, dtype=torch.int32)
        _lib.check(_lib.lib().rk_csr_schedule_upload(h, _lib.ptr(desc), _lib.stream_ptr()), "rk_csr_schedule_upload")
    finally:
        _lib.lib().rk_csr_schedule_destroy(h)
    assert np.array_equal(desc.cpu().numpy(), words)
    return desc, nb, (torch.zeros(sw, device=dev, dtype=torch.int32) if sw else None), words


def _form(dev, form):
    if form not in _sched:
        d, W, seg, pack, _ = form
        _sched[form] = _upload(dev, R.case_graph(d, W, seg)[0], R.form_split(form), d, (W, seg, pack))
        assert np.array_equal(_sched[form][3], R.form_sched(form)[0]) and _sched[form][2] is not None
    return _sched[form]


def _graph(dev, key):
    if key not in _graphs:
        rowptr, col, val, x_rows = R.case_graph(*key)
        _graphs[key] = (_t(dev, rowptr), _t(dev, col), _t(dev, val), len(rowptr) - 1, x_rows)
    return _graphs[key]


def _x(dev, key, which="x"):
    if (key, which) not in _xs:
        _xs.clear()       # one case's operands at a time: dim 256 at 16 waves is 19 MB of x
        _xs[(key, which)] = _t(dev, R.case_x(*key, which))
    return _xs[(key, which)]


def _launch(dev, form, x, x_rows=None, plain=False, scratch="own", **fields):
    """rk_spmm_csr_ex (or rk_spmm_csr) on the form's schedule -> rc"""
    desc, nb, scr, _ = _form(dev, form)
    rp, col, val, n, xr = _graph(dev, form[:3])
    scr = scr if scratch == "own" else scratch
    fields.setdefault("sum_scale", 1.0)
    head = (n, _lib.ptr(rp), _lib.ptr(col), _lib.ptr(val), _lib.ptr(desc), nb, _lib.ptr(scr), form[0], _lib.ptr(x))
    if plain:
        rc = _lib.lib().rk_spmm_csr(*head, fields.get("add"), fields["y"], _lib.stream_ptr())
    else:
        epi = _lib.SpmmEpilogue(**fields)
        rc = _lib.lib().rk_spmm_csr_ex(*head, xr if x_rows is None else x_rows, C.byref(epi), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _twice(run):
    a, b = run(), run()
    for p, q in zip(a, b):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), "not reproducible run to run"
    return a


def _same(got, want, what=""):
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def _want(form):
    d, W, _, pack, _ = form
    return R.form_walk(form, R.UNFUSED.get((d, W, pack == 1, False, False), True))


def _counters_are_zero(dev, form):
    _, _, scr, _ = _form(dev, form)
    n_long = R.form_sched(form)[3].n_long
    assert n_long >= 3 and not scr[:n_long].any().item(), "an arrival counter did not reset itself"


# the epilogue contracts: one form per dim and kernel, every W and seg among them, packed, split, generic
SUB = ((32, 16, 128, -1, 0), (64, 4, 64, -1, 0), (128, 8, 128, -1, 0), (256, 16, 64, -1, 0), (256, 4, 128, -1, 0), (32, 8, 64, 1, 0), (64, 16, 64, 1, 0),
       (128, 4, 64, 1, 0), (64, 8, 64, 1, 1), (128, 16, 128, -1, 1), (48, 16, 64, -1, 0), (100, 8, 64, -1, 0), (7, 4, 64, -1, 0), (100, 4, 128, -1, 0))
assert set(SUB) <= set(R.FORMS)
VEC = tuple(f for f in R.FORMS if f[0] in R.VEC_DIMS)


@pytest.mark.parametrize("form", R.FORMS, ids=R.form_id)
def test_no_addend_equals_the_walk_bit_for_bit(gpu_device, form):
    """through rk_spmm_csr_ex and through plain rk_spmm_csr: the same bits, the walk's"""
    n, d = len(R.case_graph(*form[:3])[0]) - 1, form[0]
    x = _x(gpu_device, form[:3])
    want = _want(form)
    for plain in (False, True):
        def run():
            y = Guarded(gpu_device, n * d)
            assert _launch(gpu_device, form, x, plain=plain, y=y.ptr) == 0, _lib.lib().rk_last_error()
            got = y.read().copy()
            assert y.untouched()
            return (got,)
        (got,) = _twice(run)
        _same(got.reshape(n, d), want, f"plain={plain}")
    _counters_are_zero(gpu_device, form)


@pytest.mark.parametrize("form", R.FORMS, ids=R.form_id)
def test_addend_is_one_more_fp32_add(gpu_device, form):
    n, d = len(R.case_graph(*form[:3])[0]) - 1, form[0]
    x = _x(gpu_device, form[:3])
    add = R.case_x(*form[:3], "add")
    add_t = _t(gpu_device, add)
    want = _want(form) + add
    for plain in (False, True):
        def run():
            y = Guarded(gpu_device, n * d)
            assert _launch(gpu_device, form, x, plain=plain, add=_lib.ptr(add_t), y=y.ptr) == 0, _lib.lib().rk_last_error()
            got = y.read().copy()
            assert y.untouched()
            return (got,)
        (got,) = _twice(run)
        _same(got.reshape(n, d), want, f"plain={plain}")
    assert np.array_equal(add_t.cpu().numpy(), add)        # the addend is only read


@pytest.mark.parametrize("form", SUB, ids=R.form_id)
def test_running_sum(gpu_device, form):
    """scales 1, 0.25 and 1 / 3; with and without y, with and without an addend"""
    n, d = len(R.case_graph(*form[:3])[0]) - 1, form[0]
    x = _x(gpu_device, form[:3])
    add, s_in = R.case_x(*form[:3], "add"), R.case_x(*form[:3], "sum_in")
    add_t, sin_t = _t(gpu_device, add), _t(gpu_device, s_in)
    walk = _want(form)
    for scale in (1.0, 0.25, 1.0 / 3.0):
        for with_add in (True, False):
            v_walk = walk + add if with_add else walk

            def run(with_y):
                y, so = Guarded(gpu_device, n * d), Guarded(gpu_device, n * d)
                rc = _launch(gpu_device, form, x, add=_lib.ptr(add_t) if with_add else None, y=y.ptr if with_y else None, sum_in=_lib.ptr(sin_t),
                             sum_out=so.ptr, sum_scale=scale)
                assert rc == 0, _lib.lib().rk_last_error()
                gy, gs = y.read().copy(), so.read().copy()
                assert so.untouched() and (y.untouched() if with_y else y.untouched(np.zeros(n * d, dtype=bool)))
                return gy, gs
            gy, gs = _twice(lambda: run(True))
            _same(gs.reshape(n, d), R.running_sum(s_in, gy.reshape(n, d), scale), (scale, with_add, "from the kernel's y"))
            _same(gy.reshape(n, d), v_walk, (scale, with_add, "y"))
            _, gs2 = _twice(lambda: run(False))
            _same(gs2.reshape(n, d), R.running_sum(s_in, v_walk, scale), (scale, with_add, "y not requested"))
    assert np.array_equal(sin_t.cpu().numpy(), s_in)
    # sum_in may be sum_out itself (the handle's running `light`)
    so = Guarded(gpu_device, n * d, fill=s_in.ravel())
    assert _launch(gpu_device, form, x, sum_in=so.ptr, sum_out=so.ptr, sum_scale=0.25) == 0
    _same(so.read().reshape(n, d), R.running_sum(s_in, walk, 0.25), "in place")
    assert so.untouched()


@pytest.mark.parametrize("form", SUB, ids=R.form_id)
def test_zeroing(gpu_device, form):
    """zero1 / zero2 become exact zeros on every row of the slab (empty rows too); zero1 may be the addend's own buffer (the train
    step's use: the addend is read before it is cleared); what is not requested keeps its sentinel"""
    n, d = len(R.case_graph(*form[:3])[0]) - 1, form[0]
    x = _x(gpu_device, form[:3])
    add = R.case_x(*form[:3], "add")

    def run(alias):
        y, z1, z2 = Guarded(gpu_device, n * d), Guarded(gpu_device, n * d, fill=add.ravel()), Guarded(gpu_device, n * d)
        a = z1 if alias else Guarded(gpu_device, n * d, fill=add.ravel())
        assert _launch(gpu_device, form, x, add=a.ptr, y=y.ptr, zero1=z1.ptr, zero2=z2.ptr) == 0, _lib.lib().rk_last_error()
        gy, g1, g2 = y.read().copy(), z1.read().copy(), z2.read().copy()
        assert y.untouched() and z1.untouched() and z2.untouched()
        assert not g1.view(np.uint32).any() and not g2.view(np.uint32).any()
        if not alias:
            assert np.array_equal(a.read(), add.ravel()) and a.untouched()
        return (gy,)
    (sep,), (ali,) = _twice(lambda: run(False)), _twice(lambda: run(True))
    _same(sep.reshape(n, d), _want(form) + add, "separate")
    _same(ali, sep, "aliased")
    # only one of the two, nothing else
    y, z1, z2 = Guarded(gpu_device, n * d), Guarded(gpu_device, n * d), Guarded(gpu_device, n * d)
    assert _launch(gpu_device, form, x, zero2=z2.ptr) == 0
    assert not z2.read().view(np.uint32).any() and z2.untouched()
    for b in (y, z1):
        b.read()
        assert b.untouched(np.zeros(n * d, dtype=bool))


@pytest.mark.parametrize("form", SUB, ids=R.form_id)
def test_adam_epilogue_equals_the_oracle_on_the_kernels_own_gradient(gpu_device, form):
    """adam_t = 1 and 1000 from the host's step number; adam_t < 0 behind rk_adam_coef_advance from a device counter at 2 (step 3)"""
    n, d = len(R.case_graph(*form[:3])[0]) - 1, form[0]
    x = _x(gpu_device, form[:3])
    add_t = _t(gpu_device, R.case_x(*form[:3], "add"))
    rng = np.random.default_rng(n * d)
    p0 = rng.standard_normal((n, d)).astype(np.float32)
    m0 = (0.01 * rng.standard_normal((n, d))).astype(np.float32)
    v0 = (0.001 * rng.random((n, d))).astype(np.float32)
    hyper = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    for t, advance in ((1, False), (1000, False), (3, True)):
        def run():
            y = Guarded(gpu_device, n * d)
            p, m, v = (Guarded(gpu_device, n * d, fill=a.ravel()) for a in (p0, m0, v0))
            coef = Guarded(gpu_device, 4)
            if advance:
                counter = torch.full((1,), t - 1, device=gpu_device, dtype=torch.int32)
                _lib.check(_lib.lib().rk_adam_coef_advance(coef.ptr, _lib.ptr(counter), 1e-3, 0.9, 0.999, _lib.stream_ptr()), "rk_adam_coef_advance")
            rc = _launch(gpu_device, form, x, add=_lib.ptr(add_t), y=y.ptr, adam_t=-1 if advance else t, adam_p=p.ptr, adam_m=m.ptr, adam_v=v.ptr,
                         coef_scratch=coef.ptr, **hyper)
            assert rc == 0, _lib.lib().rk_last_error()
            if advance:
                assert int(counter.item()) == t
            out = tuple(b.read().copy() for b in (y, p, m, v))
            assert all(b.untouched() for b in (y, p, m, v))
            coef.read()
            assert coef.untouched(np.asarray([True, True, False, False]))
            return out
        gy, gp, gm, gv = _twice(run)
        rp_, rm_, rv_ = R.adam(p0, m0, v0, gy.reshape(n, d), t)
        for name, got, ref in (("m", gm, rm_), ("v", gv, rv_), ("p", gp, rp_)):
            _same(got.reshape(n, d), ref, (name, t, advance))


@pytest.mark.parametrize("form", VEC, ids=R.form_id)
def test_src_filter_equals_the_filtered_walk(gpu_device, form):
    """every bitmap of _spmm_restate.case_hits, without an addend and with add == x (the first backward layer's t = A g + g: the
    addend of a row whose own bit is clear is not read, it is zero by the contract)"""
    d, W, seg, pack, _ = form
    rowptr, col, val, x_rows = R.case_graph(d, W, seg)
    n = len(rowptr) - 1
    xh = R.case_x(d, W, seg)
    x = _x(gpu_device, form[:3])
    s = R.form_sched(form)[3]
    fused = R.UNFUSED.get((d, W, pack == 1, False, True), True)
    for which in ("p03", "p50", "chunk", "one", "ones", "zeros"):
        hit = R.case_hits(form, which)
        bits = _t(gpu_device, R.bits_of(hit).view(np.int32))
        if which == "ones":
            want = _want(form)
        elif which == "zeros":
            want = np.zeros((n, d), dtype=np.float32)
        else:
            want = R.walk(s, rowptr, col, val, xh, fused=fused, hit=hit)
        for add_is_x in ((False, True) if which in ("p50", "one", "zeros", "ones") else (False,)):
            def run():
                y = Guarded(gpu_device, n * d)
                rc = _launch(gpu_device, form, x, add=_lib.ptr(x) if add_is_x else None, y=y.ptr, src_filter=_lib.ptr(bits))
                assert rc == 0, _lib.lib().rk_last_error()
                got = y.read().copy()
                assert y.untouched()
                return (got,)
            (got,) = _twice(run)
            w = want + np.where(hit[:n, None], xh[:n], np.float32(0.0)) if add_is_x else want
            _same(got.reshape(n, d), w, (which, add_is_x))
    _counters_are_zero(gpu_device, form)


@pytest.mark.parametrize("form", [(64, 4, 64, -1, 0), (128, 8, 64, 1, 0), (32, 16, 128, 1, 0), (256, 8, 128, -1, 0), (100, 16, 64, -1, 0)], ids=R.form_id)
def test_a_non_finite_row_nobody_references_is_never_read(gpu_device, form):
    """include/recad_hip.h: x must be finite, because padding lanes gather x[0]; a NaN / Inf row that is neither row 0 nor
    referenced (here: one more row behind the last column) leaves every output finite -- and the walk's bits"""
    d, W, seg = form[:3]
    n, x_rows = len(R.case_graph(d, W, seg)[0]) - 1, R.case_graph(d, W, seg)[3]
    xh = np.concatenate([R.case_x(d, W, seg), np.full((1, d), np.nan, dtype=np.float32)])
    xh[-1, ::2] = np.inf
    x = _t(gpu_device, xh)
    s_in = _t(gpu_device, R.case_x(d, W, seg, "sum_in"))
    hit = np.concatenate([R.case_hits(form, "p50"), [True]])
    bits = _t(gpu_device, R.bits_of(hit).view(np.int32))
    for filt in ((False, True) if d in R.VEC_DIMS else (False,)):
        y, so = Guarded(gpu_device, n * d), Guarded(gpu_device, n * d)
        rc = _launch(gpu_device, form, x, x_rows=x_rows + 1, y=y.ptr, sum_in=_lib.ptr(s_in), sum_out=so.ptr, sum_scale=0.5,
                     src_filter=_lib.ptr(bits) if filt else None)
        assert rc == 0, _lib.lib().rk_last_error()
        gy, gs = y.read().copy(), so.read().copy()
        assert np.isfinite(gy).all() and np.isfinite(gs).all() and y.untouched() and so.untouched()
        if not filt:
            _same(gy.reshape(n, d), _want(form), "y")


def test_refusals_launch_nothing(gpu_device):
    """a long-row schedule without its scratch block, sum_out without sum_in, Adam without its pointers: an error code, and every
    output keeps its sentinel"""
    form = (64, 8, 64, 1, 0)
    n, d = len(R.case_graph(*form[:3])[0]) - 1, 64
    x = _x(gpu_device, form[:3])
    outs = [Guarded(gpu_device, n * d) for _ in range(5)]
    y, so, p, m, v = outs
    coef = Guarded(gpu_device, 4)
    for what, rc in (
            ("no scratch", _launch(gpu_device, form, x, scratch=None, y=y.ptr)),
            ("no scratch, plain entry", _launch(gpu_device, form, x, scratch=None, plain=True, y=y.ptr)),
            ("sum_out without sum_in", _launch(gpu_device, form, x, y=y.ptr, sum_out=so.ptr)),
            ("Adam without p", _launch(gpu_device, form, x, y=y.ptr, adam_t=3, adam_m=m.ptr, adam_v=v.ptr, coef_scratch=coef.ptr, lr=1e-3, beta1=0.9,
                                       beta2=0.999, eps=1e-8)),
            ("Adam without its coefficient scratch", _launch(gpu_device, form, x, y=y.ptr, adam_t=3, adam_p=p.ptr, adam_m=m.ptr, adam_v=v.ptr))):
        assert rc != 0, what
        for b in outs + [coef]:
            b.read()
            assert b.untouched(np.zeros(b.n, dtype=bool)), what
    assert _launch(gpu_device, form, x, y=y.ptr) == 0
    _same(y.read().reshape(n, d), _want(form))


# ------------------------------------------------------------------------------------------ through the LightGCN handle
def _handle_graph(W, dim=64):
    """the case graph of (dim, W, 64) made square: empty rows behind it, as many rows as x has"""
    rowptr, col, val, N = R.case_graph(dim, W, 64)
    rp = np.concatenate([rowptr, np.full(N - (len(rowptr) - 1), rowptr[-1], dtype=np.int32)])
    return rp, np.asarray(col), np.asarray(val), N


def _seed(dev, graph, dim, form):
    """the forced schedule instead of the builder's choice, in the CsrGraph's cache (read when the handle is built) -> words, n_blocks"""
    desc, nb, scr, words = _upload(dev, graph.rowptr.cpu().numpy(), graph.class_split, dim, form)
    graph._sched[dim] = (desc, nb, 0 if scr is None else scr.numel())
    return words, nb


def _dropout_model(dev, W, pack, L, keep, e0, dim=64):
    from recad_amd import model
    from tests._stub import LGN_KEYS, ReplayDataset
    rp, col, val, N = _handle_graph(W, dim)
    U = N // 2
    g = dict(n_users=U, n_items=N - U, graph_row=np.repeat(np.arange(N), np.diff(rp)), graph_col=col.astype(np.int64), graph_val=val.copy(),
             batch_len=np.zeros(0, dtype=np.int64))
    ds = ReplayDataset(g, LGN_KEYS, device=dev, steps=[])
    m = model.from_config("victim", "lightgcn", latent_dim_rec=dim, lightGCN_n_layers=L, dropout=True, keep_prob=keep).I(dataset=ds)
    m._drop_seed = 0x5EED + L
    m.embedding_user.weight.data.copy_(torch.from_numpy(e0[:U]))
    m.embedding_item.weight.data.copy_(torch.from_numpy(e0[U:]))
    m = m.to(dev)
    m.use_lds, m.graph_steps = False, 0
    graph = m._csr(dev)
    assert graph is m.Graph and graph.class_split == U
    assert np.array_equal(graph.rowptr.cpu().numpy(), rp) and np.array_equal(graph.col.cpu().numpy(), col) and np.array_equal(graph.val.cpu().numpy(), val)
    words, nb = _seed(dev, graph, dim, (W, 64, pack))
    return m, R.Sched(words, nb), (rp, col, val)


def _check_dropout_light(m, s, csr, e0, L, keep, calls, fused):
    """computer() in training mode, `calls` times: each `light` is the dropout walk of every layer under that call's mask composed
    with the running-sum contract, bit for bit -> the lights"""
    rp, col, val = csr
    lights = []
    for call in range(1, calls + 1):
        lu, li = m.computer()
        got = torch.cat([lu, li]).cpu().numpy()
        assert m._drop_calls == call
        dv, kept = R.drop_values(val, DR._step_seed(m._drop_seed, (1 << 40) + call), keep)
        assert abs(kept.mean() - keep) < 0.03
        inv = np.float32(1.0) / np.float32(L + 1)
        ssum, x = e0, e0
        for l in range(1, L + 1):
            y = R.walk(s, rp, col, dv, x, fused=fused)
            ssum = R.running_sum(ssum, y, inv if l == L else np.float32(1.0))
            x = y
        _same(got, ssum, (call,))
        lights.append(got)
    return lights


@pytest.mark.parametrize("keep", [0.5, 0.9])
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("W,pack", [(4, -1), (4, 1), (8, -1), (8, 1)], ids=lambda v: str(v))
def test_dropout_propagation_through_the_handle(gpu_device, W, pack, L, keep):
    """rk_lightgcn_propagate_dropout on a forced schedule (the DROP instantiations: 4 and 8 waves, packed or not): `light` is the
    dropout walk of each layer composed with the running-sum contract, bit for bit; a second call draws another mask"""
    N = _handle_graph(W)[3]
    e0 = R._normal(np.random.default_rng([L, W]), N, 64) * np.float32(0.1)
    m, s, (rp, col, val) = _dropout_model(gpu_device, W, pack, L, keep, e0)
    assert s.W == W and (s.n_packed > 0) == (pack == 1) and s.n_long >= 3
    m.train()
    fused = R.UNFUSED.get((64, W, pack == 1, True, False), True)
    lights = _check_dropout_light(m, s, (rp, col, val), e0, L, keep, 2, fused)
    assert not np.array_equal(lights[0], lights[1])
    assert not m._ws["spmm_scratch"][:s.n_long].any().item()


@pytest.mark.parametrize("dim,W,pack", [(32, 4, -1), (32, 4, 1), (32, 8, -1), (32, 8, 1), (128, 4, -1), (128, 4, 1), (128, 8, -1), (128, 8, 1), (256, 4, -1),
                                        (256, 8, -1), (100, 4, -1), (48, 16, -1), (7, 8, -1)], ids=lambda v: str(v))
def test_dropout_propagation_at_the_other_dims(gpu_device, dim, W, pack):
    """the DROP instantiations of dims 32 / 128 / 256, and the generic kernel's dropout (any W: it has no instantiation to miss)"""
    N = _handle_graph(W, dim)[3]
    e0 = R._normal(np.random.default_rng([dim, W]), N, dim) * np.float32(0.1)
    m, s, csr = _dropout_model(gpu_device, W, pack, 1, 0.5, e0, dim)
    assert s.W == W and (s.n_packed > 0) == (pack == 1) and s.n_long >= 3
    m.train()
    _check_dropout_light(m, s, csr, e0, 1, 0.5, 1, R.UNFUSED.get((dim, W, pack == 1, True, False), True))


def test_dropout_on_16_waves_is_refused(gpu_device):
    """spmm_launch has no DROP instantiation for 16 waves: an error, `light` untouched"""
    N = _handle_graph(16)[3]
    e0 = R._normal(np.random.default_rng(16), N, 64) * np.float32(0.1)
    m, s, _ = _dropout_model(gpu_device, 16, -1, 2, 0.5, e0)
    assert s.W == 16
    m.train()
    m._ensure_handle()
    m._ws["light"].fill_(float(SENT))
    with pytest.raises(_lib.HipCallError):
        m.computer()
    torch.cuda.synchronize()
    assert (m._ws["light"] == float(SENT)).all().item()
    m.eval()                                  # ... and without dropout the same handle propagates on its 16-wave schedule
    lu, li = m.computer()
    rp, col, val, _ = _handle_graph(16)
    y1 = R.walk(s, rp, col, val, e0)
    want = R.running_sum(R.running_sum(e0, y1, 1.0), R.walk(s, rp, col, val, y1), np.float32(1.0) / np.float32(3.0))
    _same(torch.cat([lu, li]).cpu().numpy(), want)


@pytest.mark.parametrize("W,pack", [(8, 0), (4, 1)], ids=["w8", "w4-pack"])
def test_marked_block_list_same_bits_on_forced_schedules(gpu_device, W, pack):
    """tests/test_gpu_parity.py::test_lightgcn_marked_block_list_same_bits on an 8-wave schedule, and on a 4-wave one with every
    short row packed: packed waves under blk_mode 2 (the PACKED marking branch) and packed rows under row_filter"""
    from tests.test_gpu_parity import marked_block_list_same_bits
    seen = []

    def seed(m):
        graph = m._csr(m.embedding_user.weight.device)
        assert graph is m.Graph
        words, nb = _seed(m.embedding_user.weight.device, graph, m.latent_dim, (W, 0, pack))
        s = R.Sched(words, nb)
        assert s.W == W and (pack != 1 or s.n_packed > 0)
        seen.append(s)
    marked_block_list_same_bits(gpu_device, seed_schedule=seed)
    assert len(seen) == 8
