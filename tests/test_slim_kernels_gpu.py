"""GPU tests of rk_slim_fit (csrc/slim.hip) through ctypes against the numpy walk of the definition (tests/_slim_restate.py): W,
R_out and info bit for bit, with no tolerance anywhere, since the only wide operation of coordinate descent is elementwise.  G
is what rk_ease_gram wrote on the device.  Every buffer the kernel writes lies between two 64-element margins of NaN (ints: a
sentinel) that must stay as they were.  The refused matrices (a zero, a negative, an infinite and a NaN diagonal entry) are refusals
the call returns from, not faults."""
import numpy as np
import pytest
import torch

from recad_amd import _lib
from tests import _slim_restate as R
from tests.test_ease_kernels_gpu import Guarded, _bits, _gram, _P

pytestmark = pytest.mark.gpu
CAP = _lib.RK_SLIM_MAX_ITEMS


def _fit(dev, G, l1, sweeps, n=None, with_info=True, with_r=True, drop=None):
    """rk_slim_fit on G (a Guarded the device wrote, or a host array): (rc, W, info, R_out, status), the optional ones None."""
    if not isinstance(G, Guarded):
        G = Guarded(np.asarray(G).size, torch.float32, dev, init=np.asarray(G, dtype=np.float32))
    I = int(round(G.n ** 0.5))
    W, st = Guarded(I * I, torch.float32, dev), Guarded(2, torch.int32, dev)
    info = Guarded(3 * I, torch.int32, dev) if with_info else None
    Ro = Guarded(I * I, torch.float32, dev) if with_r else None
    args = [_P(G), float(l1), int(sweeps), _P(W), _P(info) if info else None, _P(Ro) if Ro else None, _P(st)]
    if drop is not None:
        args[drop] = None
    rc = _lib.lib().rk_slim_fit(I if n is None else n, *args, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert G.margins_intact()
    return rc, W, info, Ro, st


def _same(got, want, what, key):
    got, want = np.asarray(got).reshape(want.shape), np.asarray(want)
    eq = np.array_equal(_bits(got), _bits(want)) if want.dtype == np.float32 else np.array_equal(got, want)
    assert eq, (what, key, np.argwhere(got != want)[:5])


def _check_fit(dev, G_dev, fits, l1, key):
    I = int(round(G_dev.n ** 0.5))
    for sweeps, (W, Rm, info, _) in fits.items():
        rc, w, inf, ro, st = _fit(dev, G_dev, l1, sweeps)
        assert rc == 0, _lib.lib().rk_last_error()
        _same(w.host(), W, "W", key + (sweeps,))
        _same(ro.host(), Rm, "R_out", key + (sweeps,))
        _same(inf.host().reshape(I, 3), info, "info", key + (sweeps,))
        assert st.host().tolist() == [0, -1]
        assert np.all(_bits(np.diag(w.host().reshape(I, I))) == 0), "+0.0 on the diagonal"


@pytest.mark.parametrize("n", R.ITEMS)
def test_fit_equals_the_walk_bit_for_bit(gpu_device, n):
    """Every (U, l1, beta) of the table at this I, after 1, 2 and 40 sweeps, from the G the device's own rk_ease_gram wrote."""
    for case in [c for c in R.TABLE if c[0] == n]:
        _, U, l1, beta, kind = case
        c = R.case(*case)
        rc, G_dev, st = _gram(gpu_device, c["X"], beta)
        assert rc == 0, _lib.lib().rk_last_error()
        assert np.array_equal(_bits(G_dev.host().reshape(n, n)), _bits(c["G"])), "G is exactly what rk_ease_gram writes"
        _check_fit(gpu_device, G_dev, c["fits"], l1, case)


def test_every_chunk_and_stride_loop(gpu_device):
    """1100 items, three sweeps: five blocks of 256 coordinates (the last one partial), five strides of the I-wide update."""
    c = R.case(1100, 70, 1.0, 5.0, "binary", (3,))
    info = c["fits"][3][2]
    assert info[:, 0].max() == 3 and info[:, 2].sum() > 50000 and (info[:, 1] > 0).sum() > 500
    rc, G_dev, _ = _gram(gpu_device, c["X"], 5.0)
    assert rc == 0, _lib.lib().rk_last_error()
    _check_fit(gpu_device, G_dev, c["fits"], 1.0, (1100, 70))


@pytest.mark.parametrize("l1", [0.0, 1.0, 3.0])
def test_two_identical_items(gpu_device, l1):
    G = R.matrix(R.gram(R.twins()), 0.5)
    fits = R.walk(G, l1, 50, snapshots=(1, 50))
    want = np.float32(np.float32(3.0 - l1) / np.float32(3.5))
    assert fits[1][0][1, 0] == fits[1][0][0, 1] == want
    _check_fit(gpu_device, Guarded(25, torch.float32, gpu_device, init=G), fits, l1, ("twins", l1))


def test_a_residual_equal_to_l1_stays_at_zero(gpu_device):
    X = np.array([[1, 0, 1], [1, 1, 1], [0, 1, 0], [1, 1, 0]])
    G = R.matrix(R.gram(X), 0.5)
    for l1 in (2.0, 1.5):
        fits = R.walk(G, l1, 1, snapshots=(1,))
        assert (fits[1][0][0, 2] > 0) == (l1 < 2)
        _check_fit(gpu_device, Guarded(9, torch.float32, gpu_device, init=G), fits, l1, ("equal", l1))


def test_an_unrated_item_has_a_zero_row_and_column(gpu_device):
    c = R.case(65, 70, 0.0, 0.5)
    rc, w, inf, _, _ = _fit(gpu_device, c["G"], 0.0, 40)
    assert rc == 0
    W = w.host().reshape(65, 65)
    assert np.all(_bits(W[63]) == 0) and np.all(_bits(W[:, 63]) == 0) and inf.host().reshape(65, 3)[63].tolist() == [0, 0, 0] and W.any()


def test_same_call_twice_and_optional_outputs(gpu_device):
    c = R.case(257, 70, 1.0, 5.0)
    W = c["fits"][40][0]
    runs = [_fit(gpu_device, c["G"], 1.0, 40, with_info=a, with_r=b) for a, b in ((True, True), (True, True), (False, False), (True, False), (False, True))]
    for rc, w, inf, ro, st in runs:
        assert rc == 0, _lib.lib().rk_last_error()
        _same(w.host(), W, "W", ())
        assert st.host().tolist() == [0, -1]
    _same(runs[1][2].host(), runs[0][2].host(), "info", ())
    _same(runs[1][3].host(), runs[0][3].host(), "R_out", ())
    _same(runs[3][2].host(), runs[0][2].host(), "info", ())
    _same(runs[4][3].host(), runs[0][3].host(), "R_out", ())


def test_row_k_is_the_row_that_is_read(gpu_device):
    """A hand-made asymmetric G: r starts as COLUMN j and an update subtracts ROW k.  The walk on the transposed matrix is another
    result, so a kernel that read the column, or started from the row, would show."""
    rng = np.random.default_rng(5)
    n = 70
    G = rng.integers(0, 6, size=(n, n)).astype(np.float32)
    G[np.arange(n), np.arange(n)] = (rng.integers(20, 40, size=n) + 0.5).astype(np.float32)
    assert not np.array_equal(G, G.T)
    fits = R.walk(G, 1.0, 6, snapshots=(1, 6))
    other = R.walk(np.ascontiguousarray(G.T), 1.0, 6)
    assert not np.array_equal(fits[6][0], other[0]) and not np.array_equal(fits[6][0], other[0].T) and fits[6][0].any()
    _check_fit(gpu_device, Guarded(n * n, torch.float32, gpu_device, init=G), fits, 1.0, ("asymmetric",))


@pytest.mark.parametrize("kind", ["zero", "negative", "inf", "nan", "negative_zero"])
@pytest.mark.parametrize("at", [(0,), (299,), (256, 41), (7, 8, 200)])
def test_a_bad_diagonal_entry_is_refused_with_the_lowest_index(gpu_device, kind, at):
    G = R.case(300, 70, 1.0, 5.0)["G"].copy()
    for k in at:
        G[k, k] = {"zero": 0.0, "negative": -5.0, "inf": np.inf, "nan": np.nan, "negative_zero": -0.0}[kind]
    rc, w, inf, ro, st = _fit(gpu_device, G, 1.0, 3)
    assert rc == -22 and st.host().tolist() == [_lib.RK_SLIM_BAD_DIAG, min(at)], (rc, st.host())
    assert w.untouched() and inf.untouched() and ro.untouched(), "nothing is written on the refusal"
    assert f"diagonal entry {min(at)} " in _lib.lib().rk_last_error().decode()


def test_an_off_diagonal_nan_is_no_refusal(gpu_device):
    """Only the diagonal is a rule.  A NaN elsewhere spreads through r and is bounded by the loops: the call returns, and the columns
    that never read it equal the walk."""
    G = R.case(65, 70, 1.0, 5.0)["G"].copy()
    G[3, 64] = np.nan
    fits = R.walk(G, 1.0, 5, snapshots=(5,))
    rc, w, inf, ro, st = _fit(gpu_device, G, 1.0, 5)
    assert rc == 0 and st.host().tolist() == [0, -1]
    W, got = fits[5][0], w.host().reshape(65, 65)
    assert np.array_equal(np.isnan(got), np.isnan(W)) and np.array_equal(_bits(np.nan_to_num(got)), _bits(np.nan_to_num(W)))
    assert np.array_equal(inf.host().reshape(65, 3), fits[5][2])


@pytest.mark.parametrize("n,l1,sweeps,drop", [(0, 1.0, 3, None), (-1, 1.0, 3, None), (CAP + 1, 1.0, 3, None), (None, 1.0, 0, None),
                                              (None, 1.0, -2, None), (None, -1.0, 3, None), (None, -1e-30, 3, None), (None, float("nan"), 3, None),
                                              (None, float("inf"), 3, None), (None, 1.0, 3, 0), (None, 1.0, 3, 3), (None, 1.0, 3, 6)])
def test_refusals_write_nothing(gpu_device, n, l1, sweeps, drop):
    G = R.case(63, 70, 1.0, 5.0)["G"]
    rc, w, inf, ro, st = _fit(gpu_device, G, l1, sweeps, n=n, drop=drop)
    assert rc == -22 and w.untouched() and inf.untouched() and ro.untouched() and st.untouched()
    assert "rk_slim_fit" in _lib.lib().rk_last_error().decode()
