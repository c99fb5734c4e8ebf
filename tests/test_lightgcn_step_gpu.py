"""GPU tests of the LightGCN train step of the C-ABI handle (recad_amd/csrc/lightgcn.hip, rk_lightgcn_*), stage by stage and
element by element against the float64 walk and the budgets of tests/_lightgcn_step_restate.py (tests/test_lightgcn_step_host.py
shows that a correct fp32 step stays inside them and that seven planted faults do not).  The tests build _lib.LightGCNDesc
themselves, so every buffer is the test's own: each one the handle may write lies between two 64-element margins (NaN, ints a
sentinel) that must survive every call, work buffers start from garbage (3.0), loss partials from a sentinel.

Per case of the restatement's table (descriptor variant x dim x L x lambda x adam_t0) and per scatter (atomic, ordered):
  1 propagation  rk_lightgcn_propagate: every element of `light` within its budget; the isolated user's row is exactly
                 fl(E0 * fl(1 / (L + 1))) -- the kernels multiply by the fp32 reciprocal (`sum_scale`), which is fl(E0 / (L + 1))
                 bit for bit where L + 1 is a power of two, and that is asserted there as well;
  2 loss         the float64 sum of a step's 256 partials within its budget; all 256 written, later steps' slots untouched;
  3 gradient     apply_update = 0 with desc.grad: every element within its budget in row-major order, zero-budget rows (the
                 isolated user) exact zeros, tables and moments untouched bit for bit;
  4 Adam         apply_update = 1 from the same state.  Ordered scatter: the gradient is stage 3's bit for bit and p / m / v are
                 the bits of the separately rounded fp32 Adam (S.adam32, common.h adam_elem) on the gradient the call wrote, with
                 the coefficients the call left in `coef` (within an ulp of float64's) -- adam_l0_kernel at L = 0, the SpMM
                 epilogue on the row gather, pack -> sliced Adam -> unpack on the LDS path.  Atomic scatter: p, m, v within
                 their budgets given the gradient's;
  5 chaining     three one-step calls over the 96 / 96 / 77 windows (offset pointers, adam_t0 = t, t + 1, t + 2), each checked
                 from its own pre-state.  Ordered scatter: their final tables, moments and partials equal, bit for bit, one
                 three-step call with graph_steps = 0, 2, and 64 twice (the second replays the cached graph).  (The code takes ONE
                 whole-call graph for any graph_steps > 1 when the epoch has <= 64 steps -- whole_call() -- so 2 and 64 replay the
                 same three-step graph; a two-step graph plus a plain step does not exist at this size.)
  6              Atomic scatter: the three one-step calls only; the multi-step atomic call stays with the whole-table tests of
                 tests/test_gpu_parity.py;
  7 cleaning     after EVERY call gprop and gego are +0.0 in every bit (zero1 / zero2 / zero_f4_kernel / adam_l0_kernel store
                 0.f; on the LDS path with cnt and the atomic scatter gego is neither written nor cleared, it starts and stays
                 +0.0), row_bits is all zero, cnt holds the incidence counts of the call's last step alone (atomic scatter on the
                 LDS path; zeros in ordered mode, which does not count; untouched on the row gather, which must ignore it),
                 rk_lightgcn_sync_status is 0;
  8 refusals     RK_EINVAL with nothing written.

Worst |got - ref| / budget the run on an MI355X printed, over all cases (row gather / LDS path): propagate 0.333 / 0.335 with both
scatters; loss 0.0038 / 0.0036 atomic, 0.0106 / 0.0056 ordered; grad 0.113 / 0.084 atomic, 0.109 / 0.116 ordered; Adam after the
atomic scatter p 0.986 / 0.975 (the budget of p is little more than the rounding of the final subtraction, u |p|, which a
correctly rounded result comes within 2 % of on some element of a table: the fp32 restatement on the host reaches 0.985 too),
m 0.235 / 0.235, v 0.395 / 0.394.  No budget was changed after the run and no kernel fault was found: 40 of 40 tests passed the
first time."""
import ctypes as C

import numpy as np
import pytest
import torch

from recad_amd import _lib
from recad_amd.graph import CsrGraph

from . import _lightgcn_step_restate as S
from .test_ease_kernels_gpu import Guarded

pytestmark = pytest.mark.gpu
EINVAL = -22
GARBAGE = 3.0
SENT_BITS = np.float32(S.SENTINEL).view(np.uint32)
NP = _lib.RK_LOSS_PARTIALS
F32, I32 = torch.float32, torch.int32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _report(stage, where, value):
    print(f"RATIO {stage} {where} {value:.4f}")


@pytest.fixture(scope="module")
def world(gpu_device):
    """graphs on the device, their host copies, operators and triplets: built once, shared, never modified"""
    memo = {}

    def get(which, path):
        if which not in memo:
            g = S.graph(which)
            csr = CsrGraph.from_user_item_csr(g["U"], g["I"], g["r_ptr"], g["r_idx"], gpu_device)
            rowptr, col, val = (t.cpu().numpy() for t in (csr.rowptr, csr.col, csr.val))
            rp, cc = S.adjacency(g)
            assert np.array_equal(rowptr, rp) and np.array_equal(col, cc)
            hv = S.host_val(rp, cc)
            assert np.all(np.abs(val - hv) <= 2e-6 * hv)       # (what the LDS plan builder itself accepts as dinv[r] dinv[c])
            trip = S.triplets(g)
            memo[which] = {"g": g, "csr": csr, "rowptr": rowptr, "col": col, "val": val, "trip": trip,
                           "trip_dev": tuple(torch.from_numpy(a).to(gpu_device) for a in trip)}
        w = memo[which]
        if path not in w:
            w[path] = S.Operator(w["rowptr"], w["col"], w["val"], path, w["g"]["U"])
        return w, w[path]
    return get


class Handle:
    """a descriptor whose every buffer is the test's own, and the handle made from it"""

    def __init__(self, dev, w, case, ordered, grad=True, create=True):
        variant, d, L, lam, _ = case
        g, csr = w["g"], w["csr"]
        N = g["N"]
        self.dev, self.w, self.case, self.ordered, self.N, self.d, self.L = dev, w, case, ordered, N, d, L
        self.variant, self.lds = variant, variant.startswith("lds")
        self.counted = S.counted(variant, ordered)
        fbuf = lambda fill: Guarded(N * d, F32, dev, init=np.full(N * d, fill, dtype=np.float32))
        b = {k: fbuf(0.0) for k in ("p", "m", "v")}
        for k in ("buf_a", "buf_b", "light", "gprop", "gego"):
            b[k] = fbuf(GARBAGE)
        if self.counted:
            b["gego"] = fbuf(0.0)       # neither written nor cleared in this variant: it starts zero like the model's
        if grad:
            b["grad"] = fbuf(GARBAGE)
        b["state"] = Guarded(16, I32, dev, init=np.zeros(16, dtype=np.int32))
        b["coef"] = Guarded(3 * _lib.RK_MAX_GRAPH_STEPS, F32, dev, init=np.full(3 * _lib.RK_MAX_GRAPH_STEPS, S.SENTINEL, dtype=np.float32))
        b["loss"] = Guarded(3 * NP, F32, dev, init=np.full(3 * NP, S.SENTINEL, dtype=np.float32))
        words = (N + 31) // 32
        if variant in ("rg_bits", "rg_bits_cnt", "rg_blocks"):
            b["row_bits"] = Guarded(words, I32, dev, init=np.full(words, 0x5a5a5a5a, dtype=np.int32))
        if "cnt" in variant:
            b["cnt"] = Guarded(N, I32, dev, init=None if variant == "rg_bits_cnt" else np.full(N, 5, dtype=np.int32))
        wave_desc, n_blocks, plan, info = None, 0, None, _lib.LdsInfo()
        self.cap = 0
        extra = 0
        if self.lds:
            got = csr.lds_plan(d)
            assert got is not None, "the graph does not qualify for the LDS plan"
            plan, info = got
            for k in ("lsum", "e0s", "ms", "vs"):
                b[k] = fbuf(GARBAGE)
            if variant.endswith("sync"):
                b["lds_sync"] = Guarded(_lib.RK_LDS_SYNC_WORDS, I32, dev, init=np.zeros(_lib.RK_LDS_SYNC_WORDS, dtype=np.int32))
        else:
            wave_desc, n_blocks = csr.schedule(d)
            s_words = csr._sched[d][2]
            assert s_words > 0, "no long row: the scratch hand-off is not exercised"
            b["spmm_scratch"] = Guarded(s_words, I32, dev, init=np.zeros(s_words, dtype=np.int32))
            if variant == "rg_blocks":
                n_plain = int(n_blocks) & 0x07ffffff
                extra = s_words // d + 1
                self.cap = 3 * S.BATCH + extra
                assert L >= 3 and 2 * self.cap <= n_plain, "launch_forward would not take the marked-block list"
                b["row_blocks"] = Guarded(4 + n_plain, I32, dev, init=np.zeros(4 + n_plain, dtype=np.int32))
        self.b, self.keep = b, (wave_desc, plan)
        P = lambda k: _lib.ptr(b[k].mid) if k in b else None
        off = lambda k: C.c_void_p(b[k].mid.data_ptr() + 4 * g["U"] * d)
        self.desc = _lib.LightGCNDesc(
            n_users=g["U"], n_items=g["I"], dim=d, n_layers=L, lam=float(lam), lr=S.LR, beta1=S.B1, beta2=S.B2, eps=S.EPS,
            rowptr=_lib.ptr(csr.rowptr), col=_lib.ptr(csr.col), val=_lib.ptr(csr.val), wave_desc=_lib.ptr(wave_desc), n_blocks=n_blocks,
            user_emb=P("p"), item_emb=off("p"), m_user=P("m"), v_user=P("v"), m_item=off("m"), v_item=off("v"),
            buf_a=P("buf_a"), buf_b=P("buf_b"), light=P("light"), gprop=P("gprop"), gego=P("gego"), grad=P("grad"), state=P("state"), coef=P("coef"),
            spmm_scratch=P("spmm_scratch"), row_bits=P("row_bits"), row_blocks=P("row_blocks"), row_blocks_extra=int(extra),
            keep_prob=0.0, drop_seed=0, tpos=None, lds_plan=_lib.ptr(plan), lds_info=info,
            lsum=P("lsum"), e0s=P("e0s"), ms=P("ms"), vs=P("vs"), cnt=P("cnt"), lds_sync=P("lds_sync"))
        self.h = C.c_void_p()
        if create:
            _lib.check(_lib.lib().rk_lightgcn_create(C.byref(self.desc), C.byref(self.h)), "rk_lightgcn_create")
            _lib.check(_lib.lib().rk_lightgcn_set_deterministic(self.h, 1 if ordered else 0), "rk_lightgcn_set_deterministic")

    def close(self):
        if self.h:
            torch.cuda.synchronize()
            _lib.lib().rk_lightgcn_destroy(self.h)
            self.h = C.c_void_p()

    # ---- state
    def load(self, p, m, v):
        for k, a in zip("pmv", (p, m, v)):
            self.b[k].mid.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(self.dev))

    def tables(self):
        return tuple(self.b[k].host().reshape(self.N, self.d) for k in "pmv")

    def host(self, k):
        a = self.b[k].host()
        return a.reshape(self.N, self.d) if a.size == self.N * self.d else a

    def reset_loss(self, lo=0, hi=3):
        self.b["loss"].mid[lo * NP: hi * NP] = S.SENTINEL

    def snapshot(self):
        return {k: x.full.cpu().numpy().copy() for k, x in self.b.items()}

    # ---- calls
    def propagate(self):
        _lib.check(_lib.lib().rk_lightgcn_propagate(self.h, _lib.stream_ptr(self.dev)), "rk_lightgcn_propagate")
        torch.cuda.synchronize()

    def epoch_rc(self, first_step, n, adam_t0, apply_update, graph_steps=0, batch=S.BATCH, null=None, h=None):
        """rk_lightgcn_train_epoch over the n triplets from step `first_step`'s window on, partials into that step's slots"""
        u, p, q = (C.c_void_p(t.data_ptr() + 8 * first_step * S.BATCH) for t in self.w["trip_dev"])
        loss = C.c_void_p(self.b["loss"].mid.data_ptr() + 4 * first_step * NP)
        a = {"users": u, "pos": p, "neg": q, "loss": loss}
        if null:
            a[null] = None
        rc = _lib.lib().rk_lightgcn_train_epoch(self.h if h is None else h, a["users"], a["pos"], a["neg"], n, batch, adam_t0, a["loss"], apply_update, graph_steps,
                                                _lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc

    def epoch(self, *a, **k):
        _lib.check(self.epoch_rc(*a, **k), "rk_lightgcn_train_epoch")

    # ---- what must hold after every call
    def check_clean(self, last_rows=None):
        for k, x in self.b.items():
            assert x.margins_intact(), f"the margins of {k} were written"
        assert not _bits(self.b["gprop"].host()).any(), "gprop is not +0.0 everywhere after the call"
        assert not _bits(self.b["gego"].host()).any(), "gego is not +0.0 everywhere after the call"
        if "row_bits" in self.b:
            assert not self.b["row_bits"].host().any(), "row_bits is not clear after the call"
        if "cnt" in self.b:
            if not self.lds:
                assert self.b["cnt"].untouched(), "the row gather touched cnt"
            elif last_rows is not None:
                want = np.bincount(np.concatenate(last_rows), minlength=self.N) if self.counted else np.zeros(self.N, dtype=np.int64)
                assert np.array_equal(self.b["cnt"].host(), want), "cnt is not the incidence count of the last step alone"
        if "lds_sync" in self.b:
            st = C.c_int32(-1)
            _lib.check(_lib.lib().rk_lightgcn_sync_status(self.h, C.byref(st), _lib.stream_ptr(self.dev)), "rk_lightgcn_sync_status")
            assert st.value == 0, "a hand-off of the multi-phase launch timed out"
        if "row_blocks" in self.b and last_rows is not None:
            n = int(self.b["row_blocks"].host()[0])
            assert 0 < n <= self.cap, (n, self.cap)

    def partials(self, step):
        """the 256 partials of a step that ran; the slots of the steps behind it still hold the sentinel"""
        lp = self.b["loss"].host()
        mine = lp[step * NP: (step + 1) * NP]
        assert not (_bits(mine) == SENT_BITS).any() and np.all(np.isfinite(mine)), "a loss partial of the step was not written"
        return mine


SCATTERS = [pytest.param(False, id="atomic"), pytest.param(True, id="ordered")]


@pytest.mark.parametrize("ordered", SCATTERS)
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_step_stages(gpu_device, world, case, ordered):
    variant, d, L, lam, t0 = case
    w, op = world(S.graph_of(variant), S.path_of(variant))
    g = w["g"]
    where = f"{S.case_id(case)}/{'ordered' if ordered else 'atomic'}"
    start = S.state(g, d, seed=100 * d + L)
    h = Handle(gpu_device, w, case, ordered)
    try:
        h.load(*start)
        # ---- 1 propagation
        h.propagate()
        for k in h.b:
            assert h.b[k].margins_intact(), k
        light = h.host("light")
        ref_light, b_light = S.propagate64(op, start[0], L)
        r = S.ratio(light, ref_light, b_light)
        _report("propagate", where, r)
        assert r <= 1.0
        if S.graph_of(variant) == 1:
            iso = start[0][S.ISO_USER]
            want = iso if L == 0 else iso * (np.float32(1.0) / np.float32(L + 1))
            assert np.array_equal(_bits(light[S.ISO_USER]), _bits(want)), "the isolated user's row is not E0 * fl(1 / (L + 1))"
            if (L + 1) & L == 0:
                assert np.array_equal(_bits(light[S.ISO_USER]), _bits(iso / np.float32(L + 1)))
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(h.tables(), start)), "propagation wrote the tables"
        # ---- 2-7, one step after the other, each from the device's own state
        chain_partials = []
        for s in range(3):
            pre = h.tables()
            win, nb = S.window(w["trip"], s)
            rows = S.node_rows(g, win)
            t = t0 + s + 1
            ref = S.step64(op, pre[0], L, lam, rows, nb, h.counted)
            # 2 + 3: loss and gradient, no update
            h.epoch(s, nb, t0 + s, 0)
            h.check_clean(rows)
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(h.tables(), pre)), "apply_update = 0 wrote the tables or moments"
            lp0 = h.partials(s)
            assert np.all(_bits(h.b["loss"].host()[(s + 1) * NP:]) == SENT_BITS), "the partials of a step that did not run were written"
            g0 = h.host("grad")
            r_loss = abs(float(lp0.astype(np.float64).sum()) - ref["loss"]) / ref["b_loss"]
            r_grad = S.ratio(g0, ref["grad"], ref["b_grad"])
            _report("loss", where, r_loss); _report("grad", where, r_grad)
            assert r_loss <= 1.0 and r_grad <= 1.0, (s, r_loss, r_grad)
            if S.graph_of(variant) == 1:
                assert np.all(ref["b_grad"][S.ISO_USER] == 0) and not _bits(g0[S.ISO_USER]).any(), "the isolated user's gradient is not an exact zero"
            # 4: the same step with the update
            h.reset_loss(s, s + 1)
            h.b["grad"].mid.fill_(GARBAGE)
            h.epoch(s, nb, t0 + s, 1)
            h.check_clean(rows)
            lp1, g1, post = h.partials(s), h.host("grad"), h.tables()
            coef = h.host("coef")[:2]
            c64 = S.R.adam_coef(t, S.LR, S.B1, S.B2)
            assert all(abs(float(coef[k]) - c64[k]) <= float(np.spacing(np.float32(c64[k]))) for k in (0, 1)), "the step's Adam coefficients"
            if ordered:
                assert np.array_equal(_bits(g1), _bits(g0)) and np.array_equal(_bits(lp1), _bits(lp0)), "the ordered step is not reproducible"
                want = S.adam32(pre[0], g1, pre[1], pre[2], coef)
                for name, a, b in zip("pmv", post, want):
                    assert np.array_equal(_bits(a), _bits(b)), f"step {s}: {name} is not adam_elem of the gradient the call wrote"
            else:
                r_loss = abs(float(lp1.astype(np.float64).sum()) - ref["loss"]) / ref["b_loss"]
                r_grad = S.ratio(g1, ref["grad"], ref["b_grad"])
                want, bounds = S.adam64(pre[0], ref["grad"], ref["b_grad"], pre[1], pre[2], t)
                r_adam = [S.ratio(a, b, c) for a, b, c in zip(post, want, bounds)]
                _report("loss", where, r_loss); _report("grad", where, r_grad)
                for name, r in zip("pmv", r_adam):
                    _report(f"adam.{name}", where, r)
                assert max([r_loss, r_grad] + r_adam) <= 1.0, (s, r_loss, r_grad, r_adam)
            chain_partials.append(lp1)
        if not ordered:
            return
        # ---- 5: the chain against one three-step call
        final = h.tables()
        for graph_steps in (0, 2, 64, 64):
            h.load(*start)
            h.reset_loss()
            h.epoch(0, S.N_TRIP, t0, 1, graph_steps=graph_steps)
            h.check_clean(S.node_rows(g, S.window(w["trip"], 2)[0]))
            for name, a, b in zip("pmv", h.tables(), final):
                assert np.array_equal(_bits(a), _bits(b)), f"graph_steps = {graph_steps}: {name} differs from the three one-step calls"
            for s in range(3):
                assert np.array_equal(_bits(h.partials(s)), _bits(chain_partials[s])), f"graph_steps = {graph_steps}: the partials of step {s} differ"
            assert np.array_equal(_bits(h.host("grad")), _bits(g1)), "the last step's gradient differs"
    finally:
        h.close()


def test_row_gather_ignores_cnt(gpu_device, world):
    """a row-gather handle that is given cnt (launch_step sets it only on the LDS path): the bits of the run without it"""
    case_a, case_b = ("rg_bits", 64, 2, 1e-4, 7), ("rg_bits_cnt", 64, 2, 1e-4, 7)
    assert case_a in S.CASES and case_b in S.CASES
    w, _ = world(1, "rg")
    start = S.state(w["g"], 64, seed=1)
    out = []
    for case in (case_a, case_b):
        h = Handle(gpu_device, w, case, True)
        try:
            h.load(*start)
            h.epoch(0, S.N_TRIP, 7, 1)
            h.check_clean()
            out.append(h.tables() + (h.host("grad"), h.host("loss")))
            if case is case_b:
                assert h.b["cnt"].untouched()
        finally:
            h.close()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(*out)), "cnt changed what the row gather computes"


def test_refusals(gpu_device, world):
    """RK_EINVAL from check_desc and from the entry points, with nothing written"""
    w, _ = world(1, "rg")
    L_ = _lib.lib()
    rg, lds = ("rg_bits", 64, 2, 1e-4, 7), ("lds_cnt_sync", 64, 2, 1e-4, 0)
    # ---- the descriptor
    for what, case, change in (
            ("items not adjacent to users", rg, lambda x: setattr(x.desc, "item_emb", C.c_void_p(x.desc.item_emb + 4))),
            ("item moments not adjacent", rg, lambda x: setattr(x.desc, "m_item", C.c_void_p(x.desc.m_item + 4))),
            ("dim = 260", rg, lambda x: setattr(x.desc, "dim", 260)),
            ("n_users = 0", rg, lambda x: setattr(x.desc, "n_users", 0)),
            ("n_layers < 0", rg, lambda x: setattr(x.desc, "n_layers", -1)),
            ("no schedule", rg, lambda x: setattr(x.desc, "wave_desc", None)),
            ("long rows without scratch", rg, lambda x: setattr(x.desc, "spmm_scratch", None)),
            ("no workspace", rg, lambda x: setattr(x.desc, "gprop", None)),
            ("keep_prob without tpos", rg, lambda x: setattr(x.desc, "keep_prob", 0.5)),
            ("an LDS plan without lsum", lds, lambda x: setattr(x.desc, "lsum", None)),
            ("an LDS plan without vs", lds, lambda x: setattr(x.desc, "vs", None)),
            ("a misaligned lds_sync", lds, lambda x: setattr(x.desc, "lds_sync", C.c_void_p(x.desc.lds_sync + 64))),
            ("a misaligned lds_plan", lds, lambda x: setattr(x.desc, "lds_plan", C.c_void_p(x.desc.lds_plan + 4))),
            ("lds_info of another dim", lds, lambda x: setattr(x.desc.lds_info, "dim", 32))):
        x = Handle(gpu_device, w, case, False, create=False)
        before = x.snapshot()
        change(x)
        rc = L_.rk_lightgcn_create(C.byref(x.desc), C.byref(x.h))
        torch.cuda.synchronize()
        assert rc == EINVAL and not x.h and L_.rk_last_error(), what
        assert all(np.array_equal(before[k].view(np.uint32), a.view(np.uint32)) for k, a in x.snapshot().items()), what
    assert L_.rk_lightgcn_create(None, C.byref(C.c_void_p())) == EINVAL
    # ---- the entry points
    for ordered, grad in ((False, True), (False, False), (True, True)):
        x = Handle(gpu_device, w, rg, ordered, grad=grad)
        try:
            before = x.snapshot()
            calls = [("n = 0", lambda: x.epoch_rc(0, 0, 0, 1)), ("n < 0", lambda: x.epoch_rc(0, -5, 0, 1)), ("batch = 0", lambda: x.epoch_rc(0, 96, 0, 1, batch=0)),
                     ("batch < 0", lambda: x.epoch_rc(0, 96, 0, 1, batch=-1)), ("a null handle", lambda: x.epoch_rc(0, 96, 0, 1, h=C.c_void_p())),
                     ("prepare: n = 0", lambda: L_.rk_lightgcn_prepare(x.h, 0, 96, 1, 2, None)), ("prepare: batch = 0", lambda: L_.rk_lightgcn_prepare(x.h, 96, 0, 1, 2, None)),
                     ("propagate: a null handle", lambda: L_.rk_lightgcn_propagate(None, None)), ("set_deterministic: a null handle", lambda: L_.rk_lightgcn_set_deterministic(None, 1))]
            calls += [(f"null {k}", lambda k=k: x.epoch_rc(0, 96, 0, 1, null=k)) for k in ("users", "pos", "neg", "loss")]
            if not grad:
                calls += [("apply_update = 0 without desc.grad", lambda: x.epoch_rc(0, 96, 0, 0)),
                          ("prepare: apply_update = 0 without desc.grad", lambda: L_.rk_lightgcn_prepare(x.h, 96, 96, 0, 2, None))]
            if ordered:
                calls += [("prepare in deterministic mode with graph_steps > 1", lambda: L_.rk_lightgcn_prepare(x.h, S.N_TRIP, 96, 1, 2, None))]
            for what, call in calls:
                rc = call()
                torch.cuda.synchronize()
                assert rc == EINVAL and L_.rk_last_error(), what
                assert all(np.array_equal(before[k].view(np.uint32), a.view(np.uint32)) for k, a in x.snapshot().items()), what
            if ordered:     # graph_steps <= 1 is nothing to prepare: taken, and nothing written either
                assert L_.rk_lightgcn_prepare(x.h, S.N_TRIP, 96, 1, 1, None) == 0
                assert all(np.array_equal(before[k].view(np.uint32), a.view(np.uint32)) for k, a in x.snapshot().items())
        finally:
            x.close()
    # the same descriptor without a fault is taken
    x = Handle(gpu_device, w, lds, False)
    x.close()
