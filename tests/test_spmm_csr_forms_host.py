"""The row-gather SpMM's schedule with its FORM asked for (rk_csr_schedule_build_host_ex: waves 4 / 8 / 16, segments of 64 / 128,
packing forced on or off) on the CPU: the shipped builder only ever picks 4 waves below 8 M nonzeros and 8 above, so the other
forms are never built by a small test.  Over the case graphs and forms of tests/test_spmm_csr_forms_gpu.py
(tests/_spmm_restate.py):
  * the entry takes only its values, and all zero is rk_csr_schedule_build_host word for word;
  * every forced schedule keeps the structural contract (every entry in exactly one segment or packed row, segments <= seg_nnz in
    consecutive waves with the count on the leader, long rows' pieces / slots / counters, packed rows <= dim / 4 with ds.z the
    longest, the scratch formula, the 4 : 4 class interleave);
  * the fp32 walk in the kernel's order meets the float64 product per element inside (deg + 3) u sum|terms| (the budget of
    _sharded_ops_restate.spmm_ex) -- a far looser contract than the bits the GPU file demands, it only shows the walk computes A x;
  * the cases DISCRIMINATE: pieces added in reverse, a segment of a multi-segment row dropped, groups added linearly instead of by
    the butterfly, filter hits not compacted, a packed row's chain reversed -- each differs in bits from the true walk somewhere
    in the case set, so the GPU comparison cannot pass against it."""
import numpy as np
import pytest

from recad_amd import _lib
from tests import _spmm_restate as R


def _rc(rowptr, split, dim, form):
    rc, h, nb, nw, sw = R.build_handle(rowptr, split, dim, form)
    if rc == 0:
        _lib.lib().rk_csr_schedule_destroy(h)
    return rc


def test_ex_entry_takes_only_its_values():
    rowptr = R.case_graph(64, 4, 64)[0]
    for form in ((2, 0, 0), (12, 0, 0), (32, 0, 0), (-4, 0, 0), (0, 32, 0), (0, 96, 0), (0, 256, 0), (0, -64, 0), (0, 0, 2), (0, 0, -2), (4, 64, 3)):
        assert _rc(rowptr, 0, 64, form) == R.RK_EINVAL, form
        assert _lib.lib().rk_last_error().decode().startswith("rk_csr_schedule_build_host_ex:"), form
    for dim in (256, 48, 100, 7, 16):      # pack = 1 where nothing can pack
        assert _rc(rowptr, 0, dim, (0, 0, 1)) == R.RK_EINVAL, dim
        assert _lib.lib().rk_last_error().decode().startswith("rk_csr_schedule_build_host_ex:")
        assert _rc(rowptr, 0, dim, (0, 0, -1)) == 0 and _rc(rowptr, 0, dim, (16, 128, 0)) == 0
    for dim in (32, 64, 128):
        assert _rc(rowptr, 0, dim, (16, 128, 1)) == 0


@pytest.mark.parametrize("dim", [32, 64, 128, 256, 48, 7])
def test_all_zero_ex_call_is_the_shipped_schedule_word_for_word(dim):
    for key, split in (((dim, 4, 64), 0), ((64, 16, 128), 100)):
        rowptr = R.case_graph(*key)[0]
        a, b = R.build(rowptr, split, dim), R.build(rowptr, split, dim, (0, 0, 0))
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
        # ... and the shipped choice at this size is 4 waves, asked for by name
        s = R.Sched(a[0], a[1])
        assert s.W == 4
        seg = max(int(s.desc[b_, w, 2] - s.desc[b_, w, 1]) for b_ in range(s.nb) for w in range(4) if s.desc[b_, w, 3] >= 0 and s.desc[b_, w, 0] >= 0)
        c = R.build(rowptr, split, dim, (4, seg, 0))
        assert seg in (64, 128) and np.array_equal(a[0], c[0]) and a[1:] == c[1:]


@pytest.mark.parametrize("form", R.FORMS, ids=R.form_id)
def test_forced_schedule_keeps_the_structural_contract(form):
    d, W, seg, pack, _ = form
    words, nb, sw, s = R.form_sched(form)
    rowptr = R.case_graph(d, W, seg)[0]
    R.check_structure(s, rowptr, d, seg, R.form_split(form), sw)
    assert s.W == W
    deg = np.diff(rowptr)
    # the form is the one asked for: the long rows are cut into the pieces the case graph was made for, packing is all or nothing
    want_long = sorted(-(-int(k) // (W * seg)) for k in deg if k > W * seg)
    got_long = sorted(int(m[0]) for m in s.meta if m[0] > 0 and m[1] == 0)
    assert got_long == want_long and want_long[-2:] == [9, 10] and 2 in want_long
    assert s.n_packed == (int((deg <= d // 4).sum()) if pack == 1 else 0)
    # a long row's last piece of ONE entry exists (W seg + 1 and 8 W seg + 1)
    one = [b for b in range(s.nb) if s.meta[b][0] > 0 and s.meta[b][1] == s.meta[b][0] - 1 and s.desc[b][0][2] - s.desc[b][0][1] == 1 and s.desc[b][0][3] == 1]
    assert len(one) >= 2


def test_structure_check_sees_broken_schedules():
    """the checker is not vacuous: a lost entry, an oversized segment count, swapped piece indices and a wrong ds.z are each caught"""
    form = (64, 4, 64, 1, 0)
    words, nb, sw, s = R.form_sched(form)
    rowptr = R.case_graph(64, 4, 64)[0]
    o_meta = s.nb * s.W * 4 + 4

    def broken(mutate):
        w = words.copy()
        mutate(w)
        with pytest.raises(AssertionError):
            R.check_structure(R.Sched(w, nb), rowptr, 64, 64, 0, sw)
    lead = next((b, w) for b in range(s.nb) for w in range(s.W) if s.desc[b, w, 3] >= 2)
    at = (lead[0] * s.W + lead[1]) * 4
    broken(lambda w: w.__setitem__(at + 2, w[at + 2] - 1))            # an entry lost between two segments
    broken(lambda w: w.__setitem__(at + 3, w[at + 3] - 1))            # the leader counts one segment too few
    pb = [b for b in range(s.nb) if s.meta[b][0] == 10]
    broken(lambda w: (w.__setitem__(o_meta + 4 * pb[0] + 1, 1), w.__setitem__(o_meta + 4 * pb[1] + 1, 0)))   # two pieces swap their index
    pk = next((b, w) for b in range(s.nb) for w in range(s.W) if s.desc[b, w, 3] < 0)
    broken(lambda w: w.__setitem__((pk[0] * s.W + pk[1]) * 4 + 2, w[(pk[0] * s.W + pk[1]) * 4 + 2] + 1))    # ds.z is not the longest row
    with pytest.raises(AssertionError):
        R.check_structure(s, rowptr, 64, 64, 0, sw + 4)
    R.check_structure(s, rowptr, 64, 64, 0, sw)


@pytest.mark.parametrize("form", R.FORMS, ids=R.form_id)
def test_walk_meets_the_float64_product(form):
    d, W, seg = form[:3]
    rowptr, col, val, _ = R.case_graph(d, W, seg)
    x = R.case_x(d, W, seg)
    got = R.form_walk(form)
    v, mag = R.exact(rowptr, col, val, x)
    bound = (np.diff(rowptr)[:, None] + 3) * R.U32 * mag
    err = np.abs(got.astype(np.float64) - v)
    print(f"{R.form_id(form)}: worst err / bound {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
    assert (err <= bound).all()
    assert not got[np.diff(rowptr) == 0].view(np.uint32).any()      # empty rows: +0.0


@pytest.mark.parametrize("form", [(64, 4, 64, -1, 0), (32, 16, 128, 1, 0), (128, 8, 64, 1, 0), (256, 4, 128, -1, 0)], ids=R.form_id)
@pytest.mark.parametrize("which", ["p03", "p50", "chunk", "one", "ones", "zeros"])
def test_filtered_walk_meets_the_filtered_product(form, which):
    d, W, seg = form[:3]
    rowptr, col, val, _ = R.case_graph(d, W, seg)
    x = R.case_x(d, W, seg)
    hit = R.case_hits(form, which)
    got = R.walk(R.form_sched(form)[3], rowptr, col, val, x, hit=hit)
    v, mag = R.exact(rowptr, col, val, x, hit=hit)
    assert (np.abs(got - v) <= (np.diff(rowptr)[:, None] + 3) * R.U32 * mag).all()
    if which == "ones":
        assert np.array_equal(got, R.form_walk(form))
    if which == "zeros":
        assert not got.view(np.uint32).any()
    bits = R.bits_of(hit)
    assert all(bool((bits[c >> 5] >> np.uint32(c & 31)) & 1) == bool(hit[c]) for c in (0, 1, 31, 32, 63, 64, len(hit) // 3, len(hit) - 1))


def test_dropout_values_follow_the_library_mask():
    """drop_values against tests/_drop_restate._drop_keep, and a keep rate near keep_prob"""
    from tests import _drop_restate as DR
    val = R.case_graph(64, 4, 64)[2]
    for kp in (0.5, 0.9):
        seed = DR._step_seed(1234, (1 << 40) + 1)
        dv, keep = R.drop_values(val, seed, kp)
        assert np.array_equal(keep, DR._drop_keep(seed, len(val), kp))
        assert abs(keep.mean() - kp) < 0.02
        assert np.array_equal(dv[keep], val[keep] * (np.float32(1.0) / np.float32(kp))) and not dv[~keep].view(np.uint32).any()


# ---------------------------------------------------------------------------------------------- discrimination
_DISC = {"pieces_reversed": [(64, 4, 64, -1, 0), (100, 8, 64, -1, 0)], "segment_dropped": [(64, 4, 64, -1, 0), (7, 4, 64, -1, 0)],
         "groups_linear": [(32, 4, 64, -1, 0), (64, 8, 128, -1, 0)], "hits_not_compacted": [(64, 4, 64, -1, 0), (128, 8, 128, -1, 0)],
         "packed_reversed": [(64, 4, 64, 1, 0), (128, 16, 64, 1, 0)]}


@pytest.mark.parametrize("wrong", R.WRONG)
def test_cases_tell_a_wrong_order_from_the_kernels(wrong):
    """each wrong walk differs in BITS from the true one on rows of the case set -- and only on rows the mistake can reach"""
    assert set(_DISC) == set(R.WRONG) and all(f in R.FORMS for fs in _DISC.values() for f in fs)
    for form in _DISC[wrong]:
        d, W, seg, pack, _ = form
        rowptr, col, val, _ = R.case_graph(d, W, seg)
        x = R.case_x(d, W, seg)
        s = R.form_sched(form)[3]
        hit = R.case_hits(form, "p50") if wrong == "hits_not_compacted" else None
        good = R.walk(s, rowptr, col, val, x, hit=hit) if hit is not None else R.form_walk(form)
        bad = R.walk(s, rowptr, col, val, x, hit=hit, wrong=wrong)
        rows = np.nonzero((good.view(np.uint32) != bad.view(np.uint32)).any(axis=1))[0]
        deg = np.diff(rowptr)
        reach = {"pieces_reversed": deg > 2 * W * seg, "segment_dropped": deg > seg, "groups_linear": deg > 2,
                 "hits_not_compacted": deg > 1, "packed_reversed": (deg <= d // 4) & (deg > 1)}[wrong]
        print(f"{wrong} {R.form_id(form)}: {len(rows)} rows differ of {int(reach.sum())} it can reach")
        assert len(rows) >= 1 and reach[rows].all(), (wrong, form)
        if wrong in ("pieces_reversed", "segment_dropped"):
            assert len(rows) == int(reach.sum())       # every long / multi-segment row of the case tells them apart


def test_fused_and_unfused_walks_differ():
    """the `fused` flag matters: a kernel that rounded its products would not pass against the fused walk"""
    form = (64, 4, 64, -1, 0)
    a, b = R.form_walk(form), R.form_walk(form, False)
    assert (a != b).any() and np.abs(a - b).max() < 1e-4
