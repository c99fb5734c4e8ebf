"""One fp32 MFMA GEMM case through rk_gemm_f32 (include/recad_hip.h) against the oracle's k-ordered fmaf chain, shared by
tests/test_gemm_forms_gpu.py and tests/tools/gemm_forms_stress.py.

run_case() builds the operands in numpy from a seeded generator (standard_normal * 0.3: products stay far from the
denormals), lays them out in device buffers with the requested strides and base offsets (the holes of a padded operand
hold NaN: a read outside the matrix poisons the result), calls the entry, asserts the reported form and compares:

* base: orc.score_rows, the chain s = fmaf(a[k], b[k], s), k = 0..K-1;
* epilogues: single fp32 operations restated in numpy float32 in the kernels' order (biases, ReLU, mask, dropout);
* np.array_equal for everything, except
  - sigmoid (expf): the fp64 sigmoid of the bit-exact pre-activation within 3e-7 absolute,
  - split-K by atomics (order not fixed): per element |got - exact64| <= g_n (|C0| + |A| |B|^T), g_n = n u / (1 - n u),
    u = 2^-24, n = the longest slice's chain + the slices + 1 -- the textbook bound of that sum, computed in fp64.

C (and every other buffer the library writes) sits behind GUARD sentinel floats on both sides, the holes between its rows
(ldc > N) hold the sentinel too, and every float the case must not write is compared bit for bit afterwards."""
import ctypes as C

import numpy as np
import torch

from oracle import oracle as orc
from recad_amd import _lib

from ._drop_restate import _drop_keep

GUARD = 256                      # floats; 1 KiB keeps the 128-byte alignment of the allocation for the payload
SENT = np.float32(2.0 ** -60)    # small on purpose: a stray atomic add of any partial product changes its bits
U = 2.0 ** -24
RK_EINVAL = -22

NONE, SKINNY, DEEP_11_64, DEEP_12_64, DEEP_22_64, DEEP_11_32, DEEP_12_32, DEEP_22_32, WIDE_11, WIDE_12, WIDE_11_PLAIN, \
    WIDE_11_PLAIN_GROUPED, TILE128, TILE128_GATHER, TILE128_GATHER_PLAIN = range(15)
ALL_FORMS = frozenset(range(SKINNY, TILE128_GATHER_PLAIN + 1))
name_of = lambda f: _lib.RK_GEMM_FORMS[f]


class Guarded:
    """n floats on the device behind GUARD sentinel floats on both sides, shifted by `off` floats; `fill` = initial payload
    (default: the sentinel everywhere)."""

    def __init__(self, dev, n, off=0, fill=None):
        self.lo, self.n = GUARD + off, int(n)
        host = np.full(self.lo + self.n + GUARD, SENT, dtype=np.float32)
        if fill is not None:
            host[self.lo:self.lo + self.n] = fill
        self.init = host
        self.t = torch.from_numpy(host.copy()).to(dev)
        self.ptr = self.t.data_ptr() + 4 * self.lo

    def read(self):
        """copies the buffer back -> the payload (untouched() then checks the rest of this copy)"""
        self.host = self.t.cpu().numpy()
        return self.host[self.lo:self.lo + self.n]

    def untouched(self, written=None):
        """every float outside the payload positions flagged in `written` (bool[n]; default: all of the payload) still has
        its initial bits"""
        keep = np.ones(self.host.size, dtype=bool)
        if written is None:
            keep[self.lo:self.lo + self.n] = False
        else:
            keep[self.lo:self.lo + self.n] = ~written
        return np.array_equal(self.host.view(np.uint32)[keep], self.init.view(np.uint32)[keep])


class Operand:
    """mat[R, K] on the device as A(r, k) = base[r * rs + k * cs]: lay 'k' = k contiguous (cs = 1, rs = K + pad),
    'r' = rows contiguous (rs = 1, cs = R + pad); base shifted by `off` floats from an aligned address; holes are NaN."""

    def __init__(self, dev, mat, lay, pad=0, off=0):
        R, K = mat.shape
        self.rs, self.cs = (K + pad, 1) if lay == "k" else (1, R + pad)
        span = (R - 1) * self.rs + (K - 1) * self.cs + 1
        host = np.full(GUARD + off + span + GUARD, np.nan, dtype=np.float32)
        np.lib.stride_tricks.as_strided(host[GUARD + off:], (R, K), (4 * self.rs, 4 * self.cs))[...] = mat
        self.t = torch.from_numpy(host).to(dev)
        self.ptr = self.t.data_ptr() + 4 * (GUARD + off)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def call(desc):
    """rk_gemm_f32 -> (rc, form, strip form, splits)"""
    form = (C.c_int32 * 2)(-1, -1)
    splits = C.c_int32(-1)
    rc = _lib.lib().rk_gemm_f32(C.byref(desc), form, C.byref(splits), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, form[0], form[1], splits.value


def chain(A, B):
    """the k-ordered fmaf chain of every (row of A, row of B): the oracle's orc_score_rows"""
    return orc.score_rows(np.ascontiguousarray(A), np.ascontiguousarray(B))


def _kept_ok(frac):
    return 0.2 <= frac <= 0.8


def run_case(dev, M, N, K, *, form=None, strip=NONE, splits=None, seed=0, la="k", lb="k", a_pad=0, b_pad=0, a_off=0, b_off=0,
             c_off=0, ldc=None, col_bias=False, row_bias=False, const_add=0.0, relu=False, sigmoid=False, mask=False,
             ldmask=None, keep_prob=0.0, ridx=None, rmod=0, roff=0, prefix_k=0, init_base=0, split_k=0, parked=False,
             policy=0, scratch_floats=None, gates=True):
    """Runs one case and asserts everything the module docstring lists; returns (form, strip form, splits).
    form / strip / splits: the expected reports (None: not asserted -- the randomised sweep).  ridx: None, 'identity' or
    'perm' (a_ridx over a table of M + 37 rows); rmod / roff: the a_rmod row map; prefix_k > 0: acc_init, the prefix over
    prefix_k leading columns computed by a first call; parked: split-K slices into sk_part instead of atomics;
    scratch_floats: None = NULL scratch (policies 1 and 2); gates: assert that ReLU / mask keep 20-80 % of the outputs."""
    rng = np.random.default_rng([seed, M, N, K])
    f32 = lambda *shape: rng.standard_normal(shape, dtype=np.float32) * np.float32(0.3)
    ldc = N if ldc is None else ldc
    n_src = rmod if rmod else (M + 37 if ridx else M)
    Asrc, Bm = f32(n_src, K), f32(N, K)
    if ridx:
        rows = np.arange(M, dtype=np.int32) if ridx == "identity" else rng.permutation(n_src)[:M].astype(np.int32)
    elif rmod:
        rows = ((np.arange(M) + roff) % rmod).astype(np.int32)
    else:
        rows = np.arange(M, dtype=np.int32)
    Arows = Asrc[rows]
    keep = []   # device tensors the descriptor points at
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.policy = M, N, K, policy
    opa, opb = Operand(dev, Asrc, la, a_pad, a_off), Operand(dev, Bm, lb, b_pad, b_off)
    d.A, d.a_rs, d.a_cs, d.B, d.b_rs, d.b_cs = opa.ptr, opa.rs, opa.cs, opb.ptr, opb.rs, opb.cs
    if ridx:
        keep.append(_dev(rows, dev))
        d.a_ridx = keep[-1].data_ptr()
    d.a_rmod, d.a_roff = rmod, roff

    # ---- the chain, continued from a per-user prefix where the case has one
    if prefix_k:
        q = (np.arange(M) + roff) // rmod - init_base
        assert q.min() >= 0
        nq = int(q.max()) + 1
        Pu, Wu = f32(nq, prefix_k), f32(N, prefix_k)
        ld_init = N + 3
        pre = Guarded(dev, (nq - 1) * ld_init + N)
        pd = _lib.GemmDesc()
        pd.M, pd.N, pd.K = nq, N, prefix_k
        opp, opw = Operand(dev, Pu, "k"), Operand(dev, Wu, "k")
        pd.A, pd.a_rs, pd.a_cs, pd.B, pd.b_rs, pd.b_cs, pd.C, pd.ldc = opp.ptr, opp.rs, opp.cs, opw.ptr, opw.rs, opw.cs, pre.ptr, ld_init
        rc, pform, _, _ = call(pd)
        assert rc == 0, _lib.lib().rk_last_error()
        got_pre = np.lib.stride_tricks.as_strided(pre.read(), (nq, N), (4 * ld_init, 4))
        assert np.array_equal(got_pre, chain(Pu, Wu)), ("prefix", name_of(pform))
        d.acc_init, d.ld_init, d.init_base = pre.ptr, ld_init, init_base
        base = chain(np.concatenate([Pu[q], Arows], axis=1), np.concatenate([Wu, Bm], axis=1))
    elif not (split_k > 1 or policy):
        base = chain(Arows, Bm)

    # ---- epilogue operands
    cb = rb = mk = None
    if col_bias or row_bias:
        cb = f32(N)
        keep.append(_dev(cb, dev))
        d.col_bias = keep[-1].data_ptr()
    if row_bias:
        rb = f32(n_src)
        keep.append(_dev(rb, dev))
        d.row_bias = keep[-1].data_ptr()
        d.const_add = const_add
    d.relu, d.sigmoid = int(relu), int(sigmoid)
    if mask:
        ldmask = N if ldmask is None else ldmask
        mk = f32(M, N) + np.float32(0.15)      # about two thirds positive: with a ReLU in front a third of the outputs survive
        mk[rng.random((M, N)) < 0.03] = 0.0    # exact zeros are NOT kept (mask > 0)
        mkb = Operand(dev, mk, "k", ldmask - N)
        keep.append(mkb)
        d.mask, d.ldmask = mkb.ptr, ldmask
    if keep_prob:
        d.drop_thresh24 = int((1.0 - (1.0 - float(keep_prob))) * 16777216.0)   # as the entry points derive it from a dropout rate
        d.drop_scale = float(np.float32(1.0) / np.float32(keep_prob))
        d.drop_seed = 0x5EED0000 + seed

    def epilogue(s):
        """the kernels' documented order, one fp32 operation each"""
        s = s.astype(np.float32, copy=True)
        if rb is not None:
            s = ((s + rb[rows if ridx else np.arange(M)][:, None]) + cb[None, :]) + np.float32(const_add)
        elif cb is not None:
            s = s + cb[None, :]
        assert s.dtype == np.float32
        if relu:
            if gates and s.size >= 64:
                assert _kept_ok((s > 0).mean()), ("ReLU keeps", (s > 0).mean())
            s = np.where(s > 0, s, np.float32(0))
        if sigmoid:
            s = 1.0 / (1.0 + np.exp(-s.astype(np.float64)))
        if mk is not None:
            if gates and s.size >= 64:
                assert _kept_ok((mk > 0).mean()), ("mask keeps", (mk > 0).mean())
            s = np.where(mk > 0, s, 0)
        if keep_prob:
            kp = _drop_keep(d.drop_seed, M * N, keep_prob).reshape(M, N)
            s = np.where(kp, s * np.float32(d.drop_scale), np.float32(0))
        if gates and (relu or mk is not None) and s.size >= 64 and not sigmoid:
            assert _kept_ok((s != 0).mean()), ("kept outputs", (s != 0).mean())
        return s

    # ---- C behind its guards
    span = (M - 1) * ldc + N
    written = np.zeros(span, dtype=bool)
    np.lib.stride_tricks.as_strided(written, (M, N), (ldc, 1))[...] = True
    atomics = policy == 0 and split_k > 1 and not parked
    C0 = f32(M, N) if atomics else None
    fill = None
    if atomics:   # the form ADDS into C: it starts from a value that must survive
        fill = np.full(span, SENT, dtype=np.float32)
        np.lib.stride_tricks.as_strided(fill, (M, N), (4 * ldc, 4))[...] = C0
    cbuf = Guarded(dev, span, c_off, fill)
    d.C, d.ldc = cbuf.ptr, ldc
    view = lambda flat, ld=None: np.lib.stride_tricks.as_strided(flat, (M, N), (4 * (ld or ldc), 4))
    chunks = (K + 31) // 32
    what = dict(M=M, N=N, K=K, la=la, lb=lb)

    if policy == 0 and split_k > 1:
        d.split_k = split_k
        part = None
        if parked:
            sk_stride = span + 5
            part = Guarded(dev, split_k * sk_stride)
            d.sk_part, d.sk_stride = part.ptr, sk_stride
        rc, got_form, got_strip, got_splits = call(d)
        assert rc == 0, (_lib.lib().rk_last_error(), what)
        if form is not None:
            assert (got_form, got_strip) == (form, strip), (name_of(got_form), name_of(got_strip), what)
        if splits is not None:
            assert got_splits == splits, (got_splits, splits, what)
        assert 1 <= got_splits <= split_k
        per = (chunks + got_splits - 1) // got_splits
        got = cbuf.read()
        if parked and got_splits > 1:
            assert cbuf.untouched(np.zeros(span, dtype=bool)), ("C written by the parked-slices form", what)
            p1 = part.read().copy()
            wr = np.zeros(split_k * sk_stride, dtype=bool)
            for q in range(got_splits):
                wr[q * sk_stride:q * sk_stride + span] = written
                lo, hi = q * per * 32, min(K, (q + 1) * per * 32)
                assert lo < hi
                ref = chain(Arows[:, lo:hi], Bm[:, lo:hi])
                gq = view(p1[q * sk_stride:])
                assert np.array_equal(gq, ref), ("slice", q, name_of(got_form), what, np.argwhere(gq != ref)[:4])
            assert part.untouched(wr), ("parked slices wrote outside their [M, N] blocks", what)
            rc, f2, _, s2 = call(d)
            assert rc == 0 and (f2, s2) == (got_form, got_splits)
            assert np.array_equal(part.read().view(np.uint32), p1.view(np.uint32)), ("two runs differ", what)
        elif got_splits > 1:
            assert cbuf.untouched(written), ("wrote outside C[M, N]", name_of(got_form), what)
            n = min(K, per * 32) + got_splits + 1
            A64, B64 = Arows.astype(np.float64), Bm.astype(np.float64)
            exact = C0.astype(np.float64) + A64 @ B64.T
            bound = n * U / (1 - n * U) * (np.abs(C0).astype(np.float64) + np.abs(A64) @ np.abs(B64).T)
            err = np.abs(view(got).astype(np.float64) - exact)
            assert (err <= bound).all(), ("atomics", name_of(got_form), what, float((err / bound).max()), np.argwhere(err > bound)[:4])
            # the earlier value survived: without C0 the result would be off by |C0|, far outside the bound
            assert (np.abs(C0) > 4 * bound).mean() > 0.5
        else:   # one chunk of K: a single slice, the plain whole-K store
            assert cbuf.untouched(written)
            assert np.array_equal(view(got), chain(Arows, Bm)), what
        return got_form, got_strip, got_splits

    scr = None
    if policy:
        if scratch_floats is not None:
            scr = Guarded(dev, scratch_floats)
            d.scratch, d.scratch_floats = scr.ptr, scratch_floats
    rc, got_form, got_strip, got_splits = call(d)
    assert rc == 0, (_lib.lib().rk_last_error(), what)
    if form is not None:
        assert (got_form, got_strip) == (form, strip), (name_of(got_form), name_of(got_strip), what)
    if splits is not None:
        assert got_splits == splits, (got_splits, splits, what)
    if policy == 1:
        if got_splits > 1:   # the slices added in slice order in float32, then the epilogue
            per = (chunks + got_splits - 1) // got_splits
            base = None
            for q in range(got_splits):
                lo, hi = q * per * 32, min(K, (q + 1) * per * 32)
                p = chain(Arows[:, lo:hi], Bm[:, lo:hi])
                base = p if base is None else base + p
            wr = np.zeros(scratch_floats, dtype=bool)
            wr[:got_splits * M * N] = True
            scr.read()
            assert scr.untouched(wr), ("gemm_auto wrote past its slices", what)
        else:
            base = chain(Arows, Bm)
            if scr is not None:
                scr.read()
                assert scr.untouched(np.zeros(scratch_floats, dtype=bool)), ("whole-K gemm_auto touched the scratch", what)
    elif policy == 2:   # 8 consecutive k-blocks, each its own chain, combined pairwise
        assert got_splits == 8 and K % 256 == 0
        kb = K // 8
        p = [chain(Arows[:, i * kb:(i + 1) * kb], Bm[:, i * kb:(i + 1) * kb]) for i in range(8)]
        base = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))
        assert base.dtype == np.float32
        scr.read()
        assert scr.untouched()
    ref = epilogue(base)
    got = view(cbuf.read())
    assert cbuf.untouched(written), ("wrote outside C[M, N]", name_of(got_form), name_of(got_strip), what)
    if sigmoid:
        err = np.abs(got.astype(np.float64) - ref)
        assert err.max() < 3e-7, (name_of(got_form), what, err.max())
    else:
        ref = ref.astype(np.float32)
        assert np.array_equal(got, ref), (name_of(got_form), name_of(got_strip), what, "n_bad", int((got != ref).sum()),
                                          "first", np.argwhere(got != ref)[:4].tolist())
    return got_form, got_strip, got_splits
