"""GPU tests of the NCF victim's kernels (recad_amd/csrc/ncf.hip), one stage of a step at a time: rk_ncf_train_epoch and
rk_ncf_forward are driven through ctypes with descriptors the tests own, and after a call every intermediate the kernels left in
the caller's workspaces (acts, dacts, d0, grad[]) is compared, per element, with the float64 restatement of ITS stage applied to
that stage's own device inputs (tests/_pointwise_restate.py, which derives every budget by counting roundings;
tests/test_pointwise_ops_host.py shows that correct fp32 stays inside them and that six wrong implementations do not).  Each test
prints "RATIO <stage> <worst err / bound>" before it asserts <= 1; bit-exact stages report 0 or inf.  Every buffer carries a guard
band of 7.0 that must come back untouched: rows >= nb of every acts / dacts segment, d0 and out beyond their length, wgrad_part
beyond the slabs, the tail of every gradient and of the GEMM scratch.

The shapes are the smallest that reach each branch (R.NCF_CASES; test_shapes_reach_their_paths asserts that they do)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from recad_amd import _lib

from . import _pointwise_restate as R

pytestmark = pytest.mark.gpu
EINVAL = -22
GUARD = 64
SENT_BITS = np.float32(R.SENTINEL).view(np.uint32)
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def _report(r, prefix=""):
    for k, v in r.items():
        print(f"RATIO {prefix}{k} {v:.4f}")
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad


def _sent(t):
    return bool(np.all(t.cpu().numpy().view(np.uint32) == SENT_BITS))


def _same_params(got, c):
    return all(np.array_equal(R.bits(a).reshape(-1), R.bits(h).reshape(-1)) for a, h in zip(got, R.ncf_tensors(c)))


class Model:
    """device copies of a case and every workspace of rk_ncf_desc, each behind its view of a larger sentinel-filled buffer"""

    def __init__(self, dev, c, max_batch, dropout=0.0, scratch="default", drop_call=0, offset_tensor=None, state_seed=None, lr=LR, n_loss_steps=1):
        self.dev, self.c, self.mb = dev, c, max_batch
        f, L = c["f"], c["L"]
        self.w = R.widths(f, L)
        self.bufs = []
        host = [np.asarray(t, dtype=np.float32).reshape(-1) for t in R.ncf_tensors(c)]
        rng = np.random.default_rng(0 if state_seed is None else state_seed)
        self.host_m = [(0.1 * rng.standard_normal(h.size)).astype(np.float32) if state_seed is not None else np.zeros(h.size, np.float32) for h in host]
        self.host_v = [(1e-3 * rng.random(h.size) + 1e-6).astype(np.float32) if state_seed is not None else np.zeros(h.size, np.float32) for h in host]
        off = lambda k: 1 if k == offset_tensor else 0
        self.p = [self._buf(h.size, off(k), h) for k, h in enumerate(host)]
        self.g = [self._buf(h.size, off(k)) for k, h in enumerate(host)]
        self.m = [self._buf(h.size, off(k), a) for k, (h, a) in enumerate(zip(host, self.host_m))]
        self.v = [self._buf(h.size, off(k), a) for k, (h, a) in enumerate(zip(host, self.host_v))]
        self.acts, self.dacts = self._buf(max_batch * sum(self.w)), self._buf(max_batch * sum(self.w))
        self.d0 = self._buf(max_batch)
        self.n_part = ((max_batch + 63) // 64) * (2 * f + 1)
        self.wgrad_part = self._buf(self.n_part)
        self.scratch_floats = 8 * max(max_batch, 64) * self.w[0] if scratch == "default" else (scratch or 0)
        self.scratch = self._buf(self.scratch_floats) if scratch is not None else None
        self.loss = self._buf(n_loss_steps * _lib.RK_LOSS_PARTIALS)
        d = _lib.NCFDesc(n_users=c["n_users"], n_items=c["n_items"], factor=f, n_layers=L, lr=lr, beta1=B1, beta2=B2, eps=EPS,
                         ug=self.p[0].data_ptr(), ig=self.p[1].data_ptr(), um=self.p[2].data_ptr(), im=self.p[3].data_ptr(),
                         pw=self.p[4 + 2 * L].data_ptr(), pb=self.p[5 + 2 * L].data_ptr(), acts=self.acts.data_ptr(), dacts=self.dacts.data_ptr(),
                         d0=self.d0.data_ptr(), max_batch=max_batch, gemm_scratch=self.scratch.data_ptr() if self.scratch is not None else None,
                         gemm_scratch_floats=self.scratch_floats, wgrad_part=self.wgrad_part.data_ptr(), mode=c["mode"], dropout=dropout,
                         drop_seed=R.DROP_SEED, drop_call=drop_call)
        for l in range(L):
            d.W[l], d.b[l] = self.p[4 + l].data_ptr(), self.p[4 + L + l].data_ptr()
        for t in range(len(host)):
            d.grad[t], d.m[t], d.v[t] = self.g[t].data_ptr(), self.m[t].data_ptr(), self.v[t].data_ptr()
        self.desc = d
        self.users, self.items, self.labels = (torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("users", "items", "labels"))

    def _buf(self, n, off=0, init=None):
        """a view of n floats, `off` floats into a buffer of n + off + GUARD sentinels"""
        whole = torch.full((n + off + GUARD,), R.SENTINEL, device=self.dev)
        view = whole[off:off + n]
        if init is not None:
            view.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32).reshape(-1)))
        self.bufs.append((whole, off, n))
        return view

    def guards_intact(self):
        return all(_sent(whole[:off]) and _sent(whole[off + n:]) for whole, off, n in self.bufs)

    def train(self, n=None, batch=None, adam_t0=0, apply=0, lo=0):
        n = len(self.c["users"]) - lo if n is None else n
        ptr = lambda t: C.c_void_p(t.data_ptr() + 8 * lo)
        rc = _lib.lib().rk_ncf_train_epoch(C.byref(self.desc), ptr(self.users), ptr(self.items), ptr(self.labels), n, n if batch is None else batch,
                                           adam_t0, _lib.ptr(self.loss), apply, _lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc

    def forward(self, n=None, user_ids=None, n_items=0, users=None, items=None):
        users, items = (self.users if users is None else users), (self.items if items is None else items)
        n = len(users) if n is None else n
        out = torch.full((n + GUARD,), R.SENTINEL, device=self.dev)
        rc = _lib.lib().rk_ncf_forward(C.byref(self.desc), None if user_ids is not None else _lib.ptr(users), None if user_ids is not None else _lib.ptr(items),
                                       _lib.ptr(user_ids), n_items, n, _lib.ptr(out), _lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[n:].view(np.uint32) == SENT_BITS), "written past out[n]"
        return rc, got[:n]

    def segments(self, buf, nb, written=None):
        """[nb, w_l] of every segment; the rows from nb on (from `written` on after a call of several chunks) must hold the sentinel"""
        a, out, o = buf.cpu().numpy(), [], 0
        for w in self.w:
            seg = a[o:o + self.mb * w].reshape(self.mb, w)
            assert np.all(seg[nb if written is None else written:].view(np.uint32) == SENT_BITS), "a row >= nb of an activation segment was written"
            out.append(seg[:nb].copy())
            o += self.mb * w
        return out

    def workspace(self, nb, step=0):
        gmf = self.c["mode"] == R.GMF
        if gmf:
            assert _sent(self.acts) and _sent(self.dacts), "GMF has no tower"
        d0 = self.d0.cpu().numpy()
        assert np.all(d0[nb:].view(np.uint32) == SENT_BITS)
        part = self.wgrad_part.cpu().numpy()
        used = math.ceil(nb / R.WGRAD_SLAB) * (R.ps_of(self.c["f"], self.c["mode"]) + 1)
        assert np.all(part[used:].view(np.uint32) == SENT_BITS) and not np.any(part[:used].view(np.uint32) == SENT_BITS), "wgrad_part: not exactly the slabs were written"
        loss = self.loss.cpu().numpy()[step * 256:(step + 1) * 256]
        assert self.guards_intact(), "a guard band was written"
        return {"acts": [None] * (len(self.w)) if gmf else self.segments(self.acts, nb), "dacts": [None] * len(self.w) if gmf else self.segments(self.dacts, nb),
                "d0": d0[:nb].copy(), "grad": [g.cpu().numpy() for g in self.g], "loss": float(loss.astype(np.float64).sum()), "loss_row": loss.copy()}

    def state(self):
        return [[t.cpu().numpy() for t in ts] for ts in (self.p, self.m, self.v, self.g)]


# ================================================================ one step, stage by stage
@pytest.mark.parametrize("name", list(R.NCF_CASES))
def test_step_stages(gpu_device, name):
    c = R.named_case(name)
    f, L, mode, nb, p = R.NCF_CASES[name]
    m = Model(gpu_device, c, max_batch=nb + 5, dropout=p)
    assert m.train(adam_t0=3) == 0, _lib.lib().rk_last_error()
    ws = m.workspace(nb)
    _report(R.check_ncf_step(c, ws, (p, R.DROP_SEED, 3) if p > 0 else None), prefix=f"{name}.")
    params = m.state()[0]
    assert _same_params(params, c), "apply_update = 0 moved a parameter"


def test_blocked_forward_in_row_chunks_gives_the_same_bits(gpu_device):
    """case C': a scratch of 8 * 128 * 256 floats makes gemm_fwd_blocked take layer 0 (200 x 256 x 512) in row chunks of 128 + 72"""
    c = R.named_case("C")
    nb = 200
    cap = 8 * 128 * 256
    assert min(nb, cap // (8 * 256) // 64 * 64) == 128 and min(nb, cap // (8 * 128) // 64 * 64) == nb
    whole, chunked = Model(gpu_device, c, max_batch=nb + 5), Model(gpu_device, c, max_batch=nb + 5, scratch=cap)
    assert whole.scratch_floats >= 8 * nb * 256
    assert whole.train() == 0 and chunked.train() == 0, _lib.lib().rk_last_error()
    a, b = whole.workspace(nb), chunked.workspace(nb)
    _report(R.check_ncf_step(c, b), prefix="C'.")
    for l in range(c["L"] + 1):
        assert np.array_equal(R.bits(a["acts"][l]), R.bits(b["acts"][l])), f"acts[{l}] differs between one chunk and two"


def _gemm_query(dev, M, N, K, policy, scratch_floats, **kw):
    A, B, Cm, scratch = kw.pop("A"), kw.pop("B"), torch.empty(M, N, device=dev), torch.empty(scratch_floats, device=dev)
    d = _lib.GemmDesc(M=M, N=N, K=K, policy=policy, A=A.data_ptr(), B=B.data_ptr(), C=Cm.data_ptr(), ldc=N, scratch=scratch.data_ptr(),
                      scratch_floats=scratch_floats, **kw)
    form, splits = (C.c_int32 * 2)(), C.c_int32(0)
    rc = _lib.lib().rk_gemm_f32(C.byref(d), form, C.byref(splits), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().rk_last_error()
    return splits.value


def test_shapes_reach_their_paths(gpu_device):
    dev = gpu_device
    # case C, layer 1's dX: dY [200, 128] . W1 [128, 256] under the mask of acts[1], K-sliced
    nb, cap = 200, 8 * 205 * 512
    dy, W1, mask = torch.randn(nb, 128, device=dev), torch.randn(128, 256, device=dev), torch.randn(nb, 256, device=dev)
    assert _gemm_query(dev, nb, 256, 128, _lib.RK_GEMM_POLICY_AUTO, cap, A=dy, a_rs=128, a_cs=1, B=W1, b_rs=1, b_cs=256, mask=mask.data_ptr(), ldmask=256) > 1
    assert _gemm_query(dev, nb, 256, 128, _lib.RK_GEMM_POLICY_AUTO, 8 * 128 * 256, A=dy, a_rs=128, a_cs=1, B=W1, b_rs=1, b_cs=256, mask=mask.data_ptr(), ldmask=256) > 1
    x, W0, b0 = torch.randn(nb, 512, device=dev), torch.randn(256, 512, device=dev), torch.randn(256, device=dev)
    assert _gemm_query(dev, nb, 256, 512, _lib.RK_GEMM_POLICY_FWD_BLOCKED, 8 * 128 * 256, A=x, a_rs=512, a_cs=1, B=W0, b_rs=512, b_cs=1, col_bias=b0.data_ptr(), relu=1) == 8
    # the shape arithmetic of the other rows of the case table
    w = lambda name: R.widths(*R.NCF_CASES[name][:2])
    assert [k % 256 == 0 for k in w("B")[:-1]] == [True] * 3 + [False] * 5 and w("B")[0] // 2 == 512 > 256, "B: blocked forward at layers 0..2, two trips of the gather's lane loop"
    assert len(R.tensor_sizes(9, 9, 4, 8, R.MLP)) == 22
    assert [k % 256 == 0 for k in w("C")[:-1]] == [True, True, False] and R.ps_of(64, R.NEUMF) + 1 == 129 and math.ceil(200 / 64) == 4 and 200 % 64 == 8 and 200 > 128
    assert R.NCF_CASES["Dmlp"][3] > 1024 and math.ceil(1100 / 64) == 18 and R.loss_trips(1100) == 2
    assert R.ps_of(64, R.MLP) + 1 == 65 and R.ps_of(4, R.NEUMF) + 1 == 9
    assert [math.ceil(nb / 64) for nb in (64, 65)] == [1, 2]


# ================================================================ Adam and the epoch loop
def _adam_case(f, L, mode, n_users, nb=32, seed=11):
    return R.ncf_case(f, L, mode, nb, seed=seed, n_users=n_users, hubs=False)


def _oracle_adam(p, g, m, v, t, lr=LR):
    p, m, v = (np.ascontiguousarray(a, dtype=np.float32).copy() for a in (p, m, v))
    orc.adam(p, np.ascontiguousarray(g, dtype=np.float32), m, v, t, lr, B1, B2, EPS)
    return p, m, v


@pytest.mark.parametrize("shape", ["two_quads", "tail"])
@pytest.mark.parametrize("adam_t0", [0, 999])
def test_fused_adam_step_is_the_oracles_bits(gpu_device, shape, adam_t0):
    if shape == "two_quads":     # um: 4200 * 256 floats > 2^20: two quads in flight, the grid at its cap
        c = _adam_case(64, 3, R.NEUMF, 4200)
        assert 4200 * 256 // 4 > 1024 * 256 and min((4200 * 256 // 4 + 255) // 256 + 1, 1024) == 1024
        offsets = (None, 0)      # tensor 0 (ug: read by scalar loads only) one float off 16 bytes: the scalar path
    else:                        # GMF, factor 6: pw has 6 entries, pb 1, the tables n * 6
        c = _adam_case(6, 2, R.GMF, 41)
        assert (6 << 1) % 4 == 0 and R.tensor_sizes(41, 38, 6, 2, R.GMF)[-2:] == [6, 1] and (41 * 6) % 4 != 0
        offsets = (None,)
    nb = c["nb"]
    assert len(np.unique(c["users"])) == nb and len(np.unique(c["items"])) == nb and nb <= 32
    results = []
    for off in offsets:
        grads = []
        for _ in range(2):      # the gradients do not depend on atomic order: one incidence per row, dW unsplit
            m = Model(gpu_device, c, max_batch=nb + 5, offset_tensor=off, state_seed=7)
            assert m.train(adam_t0=adam_t0) == 0, _lib.lib().rk_last_error()
            grads.append(m.state()[3])
        assert all(np.array_equal(R.bits(a), R.bits(b)) for a, b in zip(*grads)), "two apply_update = 0 runs differ"
        if off is not None:
            assert m.p[off].data_ptr() % 16 == 4 and m.g[off].data_ptr() % 16 == 4
        m = Model(gpu_device, c, max_batch=nb + 5, offset_tensor=off, state_seed=7)
        assert m.train(adam_t0=adam_t0, apply=1) == 0, _lib.lib().rk_last_error()
        assert m.guards_intact()
        p, mm, vv, g = m.state()
        for k, (h, g0) in enumerate(zip(R.ncf_tensors(c), grads[0])):
            want = _oracle_adam(h.reshape(-1), g0, m.host_m[k], m.host_v[k], adam_t0 + 1)
            for name, a, b in zip("pmv", (p[k], mm[k], vv[k]), want):
                assert np.array_equal(R.bits(a), R.bits(b)), (shape, "tensor", k, name, "offset", off)
            assert not np.any(R.bits(g[k])), "a gradient is not +0.0 after the update"
        results.append((p, mm, vv))
    if len(results) == 2:
        assert all(np.array_equal(R.bits(a), R.bits(b)) for x, y in zip(*results) for a, b in zip(x, y)), "the scalar path differs from the vector path"


def test_epoch_numbers_masks_steps_and_the_short_tail(gpu_device):
    """lr = 0 keeps the parameters' bits, so the three steps (32, 32, 16 pairs, dropout 0.3) see one model: the moments after the
    epoch are the oracle's Adam chain over the gradients of three separate apply_update = 0 calls with adam_t0 + s"""
    f, L, p, t0, n, B = 8, 2, 0.3, 5, 80, 32
    c = R.ncf_case(f, L, R.NEUMF, n, seed=21, hubs=False)
    m = Model(gpu_device, c, max_batch=B, dropout=p, state_seed=3, lr=0.0, n_loss_steps=3)
    assert m.train(n=n, batch=B, adam_t0=t0, apply=1) == 0, _lib.lib().rk_last_error()
    assert m.guards_intact()
    P, M, V, G = m.state()
    epoch_loss = m.loss.cpu().numpy().reshape(3, 256)
    assert _same_params(P, c), "lr = 0 moved a parameter"
    want_m, want_v = [a.copy() for a in m.host_m], [a.copy() for a in m.host_v]
    for s, (lo, hi) in enumerate(((0, 32), (32, 64), (64, 80))):
        one = Model(gpu_device, c, max_batch=B, dropout=p)
        assert one.train(n=hi - lo, batch=B, adam_t0=t0 + s, lo=lo) == 0, _lib.lib().rk_last_error()
        sub = R.sub_case(c, lo, hi)
        ws = one.workspace(hi - lo)
        _report(R.check_ncf_step(sub, ws, (p, R.DROP_SEED, t0 + s)), prefix=f"epoch.step{s}.")
        assert np.array_equal(R.bits(epoch_loss[s]), R.bits(ws["loss_row"])), f"loss row {s} of the epoch differs from the step on its own"
        for k, g in enumerate(ws["grad"]):
            _, want_m[k], want_v[k] = _oracle_adam(R.ncf_tensors(c)[k].reshape(-1), g, want_m[k], want_v[k], t0 + s + 1, lr=0.0)
    for k in range(len(M)):
        assert np.array_equal(R.bits(M[k]), R.bits(want_m[k])) and np.array_equal(R.bits(V[k]), R.bits(want_v[k])), ("tensor", k)
        assert not np.any(R.bits(G[k]))


# ================================================================ rk_ncf_forward
def test_forward_explicit_pairs_in_chunks(gpu_device):
    c = R.ncf_case(8, 2, R.NEUMF, 250, seed=31)
    one = Model(gpu_device, c, max_batch=256)
    rc, whole = one.forward()
    assert rc == 0, _lib.lib().rk_last_error()
    acts = one.segments(one.acts, 250)
    _report(R.check_ncf_forward(c, {"acts": acts, "logits": whole}), prefix="forward.pairs250.")
    three = Model(gpu_device, c, max_batch=96)
    rc, chunked = three.forward()
    assert rc == 0 and np.array_equal(R.bits(chunked), R.bits(whole)), "chunks of 96, 96, 58 differ from one chunk"
    assert one.guards_intact() and three.guards_intact() and _sent(one.dacts) and _sent(one.d0)


def test_forward_second_trip_of_the_scoring_grid(gpu_device):
    c = R.ncf_case(4, 1, R.NEUMF, 4200, seed=32)
    assert 4200 > 4 * 1024
    m = Model(gpu_device, c, max_batch=4200)
    rc, out = m.forward()
    assert rc == 0, _lib.lib().rk_last_error()
    _report(R.check_ncf_forward(c, {"acts": m.segments(m.acts, 4200), "logits": out}), prefix="forward.pairs4200.")
    assert m.guards_intact()


@pytest.mark.parametrize("mode", [R.NEUMF, R.MLP, R.GMF])
def test_forward_full_catalogue_chunks_begin_inside_a_user(gpu_device, mode):
    I, mb = 37, 100
    ids = np.array([3, 11, 0, 11, 40, 7, 22], dtype=np.int32)
    n = len(ids) * I
    assert (100 // I, 100 % I) == (2, 26) and (200 // I, 200 % I) == (5, 15)
    c = R.ncf_case(8, 2, mode, 5, seed=33 + mode, n_users=41, n_items=I)
    users = torch.from_numpy(np.repeat(ids.astype(np.int64), I)).to(gpu_device)
    items = torch.from_numpy(np.tile(np.arange(I, dtype=np.int64), len(ids))).to(gpu_device)
    ids_t = torch.from_numpy(ids).to(gpu_device)
    pairs = Model(gpu_device, c, max_batch=mb)
    rc, want = pairs.forward(users=users, items=items)
    assert rc == 0, _lib.lib().rk_last_error()
    sub = dict(c, users=np.repeat(ids.astype(np.int64), I)[200:], items=np.tile(np.arange(I), len(ids))[200:])
    if mode != R.GMF:       # the last chunk of the explicit run, stage by stage
        _report(R.check_ncf_forward(sub, {"acts": pairs.segments(pairs.acts, n - 200, written=mb), "logits": want[200:]}), prefix=f"forward.catalogue.{R.MODE_NAMES[mode]}.")
    out0 = R.widths(8, 2)[0] // 2
    for what, kw in (("prefix", {}), ("no scratch: the gather path", dict(scratch=None)), ("scratch below users x out0: prefix refused", dict(scratch=len(ids) * out0 - 1))):
        m = Model(gpu_device, c, max_batch=mb, **kw)
        rc, got = m.forward(n=n, user_ids=ids_t, n_items=I)
        assert rc == 0, (what, _lib.lib().rk_last_error())
        assert np.array_equal(R.bits(got), R.bits(want)), f"full catalogue ({what}) differs from the explicit pairs"
        assert m.guards_intact(), what
        if mode != R.GMF:
            m.segments(m.acts, n - 200, written=mb)
            if what == "prefix":      # neither the gather nor the [pairs, 2E] input exist on this path
                assert _sent(m.acts[:mb * m.w[0]])


def test_forward_dropout_masks_are_numbered_by_call_and_chunk(gpu_device):
    c = R.ncf_case(8, 3, R.NEUMF, 250, seed=34)
    p, mb = 0.3, 96
    m = Model(gpu_device, c, max_batch=mb, dropout=p, drop_call=5)
    rc, out = m.forward()
    assert rc == 0, _lib.lib().rk_last_error()
    last = R.sub_case(c, 192, 250)
    _report(R.check_ncf_forward(last, {"acts": m.segments(m.acts, 58, written=mb), "logits": out[192:]}, (p, R.DROP_SEED, R.score_call(5, 2))), prefix="forward.dropout.")
    other = Model(gpu_device, c, max_batch=mb, dropout=p, drop_call=6)
    rc, out2 = other.forward()
    assert rc == 0 and not np.array_equal(out, out2), "two drop_call values give the same scores"
    again = Model(gpu_device, c, max_batch=mb, dropout=p, drop_call=5)
    assert np.array_equal(R.bits(again.forward()[1]), R.bits(out))


def test_refusals_launch_nothing(gpu_device):
    nb = 20

    def refused(what, train=True, case=None, batch=None, edit=None, **kw):
        m = Model(gpu_device, case or R.ncf_case(8, 2, R.NEUMF, nb, seed=35), max_batch=kw.pop("max_batch", nb), **kw)
        if edit:
            edit(m.desc)
        rc, out = (m.train(batch=batch), None) if train else m.forward()
        assert rc == EINVAL and _lib.lib().rk_last_error(), what
        assert out is None or np.all(out.view(np.uint32) == SENT_BITS), what
        assert m.guards_intact() and all(_sent(t) for t in (m.acts, m.dacts, m.d0, m.wgrad_part, m.loss) + tuple(m.g)), what
        assert _same_params(m.state()[0], m.c), what

    def unset(field, k=None):
        def edit(d):
            if k is None:
                setattr(d, field, None)
            else:
                getattr(d, field)[k] = None
        return edit
    refused("batch > max_batch", max_batch=nb - 1, batch=nb)
    for field in ("grad", "m", "v"):
        refused(f"{field}[5] missing", edit=unset(field, 5))
    refused("wgrad_part missing", edit=unset("wgrad_part"))
    refused("an unknown mode", edit=lambda d: setattr(d, "mode", 3))
    refused("an unknown mode in scoring", train=False, edit=lambda d: setattr(d, "mode", -1))
    refused("dropout = 1", edit=lambda d: setattr(d, "dropout", 1.0))
    refused("n_layers = 9", edit=lambda d: setattr(d, "n_layers", 9))
    refused("factor * 2^(L - 1) % 4 != 0", edit=lambda d: setattr(d, "factor", 3))
    refused("K % 256 == 0 without a scratch in training", case=R.ncf_case(64, 2, R.MLP, nb, seed=36), scratch=None)
    # the same calls without the fault are taken
    m = Model(gpu_device, R.ncf_case(8, 2, R.NEUMF, nb, seed=35), max_batch=nb)
    assert m.train() == 0 and m.forward()[0] == 0
