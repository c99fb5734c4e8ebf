"""GPU tests of the APR victim's kernels (recad_amd/csrc/apr.hip) through rk_apr_train_epoch: every case of the table of
tests/_apr_restate.py as a one-step epoch, each stage read out of the workspace behind sentinel prefills and compared with the
restatement of THAT stage fed the device's own inputs -- x, c, the norms, Delta, x', c' and the losses within their counted budgets,
Gamma and the gradient rows bit for bit against the fp32 walk in key order, slot_of, the run table and the sorted keys exactly, Adam
bit for bit against the oracle's -- then the epoch loop (a short last step, Adam's step numbering against the chained oracle), the switches (apply_update = 0,
adv_reg = 0, eps = 0, lr = 0), repeatability, and the refusals.  Each test prints "RATIO <stage> <worst err / bound>" before it
asserts <= 1."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from recad_amd import _lib

from . import _apr_restate as R

pytestmark = pytest.mark.gpu
EINVAL = -22
GUARD = 64
SENT_BITS = np.float32(R.SENTINEL).view(np.uint32)
LR, B1, B2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8
IDS = [f"d{d}-B{B}-{k}" for d, B, k in R.CASES]
STEP_AREAS = ("slot_of", "gamma", "norm", "delta", "x_adv", "c_adv")          # what steps 2-4 write


def _same(a, b):
    return np.array_equal(R.bits(a).reshape(-1), R.bits(b).reshape(-1))


def _report(r, prefix=""):
    for k, v in r.items():
        print(f"RATIO {prefix}{k} {v:.4f}")
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad


class Apr:
    """device buffers of one call, every one between two margins of GUARD sentinel words"""

    def __init__(self, dev, c, n=None, batch=None, state_seed=None, lo=0):
        self.dev, self.c, self.lo = dev, c, lo
        self.U, self.I, self.d = c["U"], c["I"], c["d"]
        self.N = self.U + self.I
        self.n = len(c["u"]) - lo if n is None else n
        self.batch = self.n if batch is None else batch
        self.n_steps = (self.n + self.batch - 1) // self.batch
        self.bufs = []
        tot = self.N * self.d
        rng = np.random.default_rng(0 if state_seed is None else state_seed)
        self.host_m = (0.1 * rng.standard_normal(tot)).astype(np.float32) if state_seed is not None else np.zeros(tot, np.float32)
        self.host_v = (1e-3 * rng.random(tot) + 1e-6).astype(np.float32) if state_seed is not None else np.zeros(tot, np.float32)
        self.tab, self.m, self.v, self.g = self._buf(tot, c["tab"]), self._buf(tot, self.host_m), self._buf(tot, self.host_v), self._buf(tot)
        self.losses = self._buf(2 * 3 * self.n_steps)                      # doubles, as pairs of sentinel words
        self.status = self._buf(2)
        self.ids = [torch.from_numpy(np.ascontiguousarray(c[k], dtype=np.int64)).to(dev) for k in ("u", "i", "j")]
        self.lay = _lib.AprLayout()
        rc = _lib.lib().rk_apr_workspace(self.U, self.I, self.d, self.n, self.batch, C.byref(self.lay))
        assert rc == 0, _lib.lib().rk_last_error()
        assert self.lay.bytes % 256 == 0 and all(getattr(self.lay, k) % 256 == 0 for k in _lib.AprLayout.AREAS if k != "sort_tmp_bytes")
        self.ws = self._buf(self.lay.bytes // 4)
        assert self.ws.data_ptr() % 256 == 0

    def _buf(self, n, init=None):
        whole = torch.full((n + 2 * GUARD,), R.SENTINEL, device=self.dev, dtype=torch.float32)
        if init is not None:
            whole[GUARD:GUARD + n].copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32).reshape(-1)))
        self.bufs.append((whole, n))
        return whole[GUARD:GUARD + n]

    def guards_intact(self):
        return all(bool(np.all(np.r_[w[:GUARD].cpu().numpy(), w[GUARD + n:].cpu().numpy()].view(np.uint32) == SENT_BITS)) for w, n in self.bufs)

    def run(self, adam_t0=0, apply=1, lr=LR, **over):
        c = self.c
        a = dict(n_users=self.U, n_items=self.I, dim=self.d, table=self.tab, m=self.m, v=self.v, grad=self.g, lam=c["lam"], eps=c["eps"],
                 adv_reg=c["adv_reg"], workspace=self.ws, workspace_bytes=self.lay.bytes, n=self.n, batch=self.batch, users=self.ids[0],
                 pos=self.ids[1], neg=self.ids[2], losses=self.losses, status=self.status, desc=True)
        a.update(over)
        p = lambda t: None if t is None else t.data_ptr()
        desc = _lib.AprDesc(n_users=a["n_users"], n_items=a["n_items"], dim=a["dim"], table=p(a["table"]), m=p(a["m"]), v=p(a["v"]),
                            grad=p(a["grad"]), lam=a["lam"], eps=a["eps"], adv_reg=a["adv_reg"], lr=lr, beta1=B1, beta2=B2, adam_eps=ADAM_EPS,
                            workspace=p(a["workspace"]), workspace_bytes=a["workspace_bytes"])
        ids = lambda t: None if t is None else C.c_void_p(t.data_ptr() + 8 * self.lo)
        rc = _lib.lib().rk_apr_train_epoch(C.byref(desc) if a["desc"] else None, ids(a["users"]), ids(a["pos"]), ids(a["neg"]), a["n"], a["batch"],
                                           adam_t0, apply, _lib.ptr(a["losses"]), _lib.ptr(a["status"]), _lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc

    # ---- reading
    def area(self, name, dtype, count):
        raw = self.ws.cpu().numpy().view(np.uint8)
        o = getattr(self.lay, name)
        return raw[o:o + count * np.dtype(dtype).itemsize].view(dtype).copy()

    def words_outside(self, written):
        """the workspace's 32-bit words with the byte ranges of `written` ({area: bytes}) blanked to the sentinel: all that remains
        must be the prefill (the sort's scratch and input are the library's to use)"""
        raw = self.ws.cpu().numpy().view(np.uint32).copy()
        for name, nbytes in dict(written, keys_in=8 * 3 * self.n, sort_tmp=self.lay.sort_tmp_bytes).items():
            o = getattr(self.lay, name)
            raw[o // 4:(o + nbytes + 3) // 4] = SENT_BITS
        return raw

    def step_losses(self):
        return self.losses.cpu().numpy().view(np.float64).reshape(self.n_steps, 3)

    def host(self, t):
        return t.cpu().numpy()

    def triplets(self):
        c, lo = self.c, self.lo
        return c["u"][lo:lo + self.n], c["i"][lo:lo + self.n], c["j"][lo:lo + self.n]


def _written(a, n_slots, adv=True):
    """bytes of each area a ONE-step call writes"""
    nb, d = a.n, a.d
    w = {"keys": 8 * 3 * nb, "run": 4 * (n_slots + 2), "x": 4 * nb, "c": 4 * nb, "part": 8 * 3 * a.lay.part_blocks, "grad": 4 * a.N * d}
    if adv:
        w.update({"slot_of": 4 * 3 * nb, "gamma": 4 * n_slots * d, "norm": 4 * n_slots, "delta": 4 * n_slots * d, "x_adv": 4 * nb, "c_adv": 4 * nb})
    return w


def _stages(a, pl, adv=True):
    """what a one-step call left in the workspace, the losses and desc.grad"""
    ns, nb, d = len(pl["rows"]), a.n, a.d
    L, La, Rg = a.step_losses()[0]
    got = {"x": a.area("x", np.float32, nb), "c": a.area("c", np.float32, nb), "L": float(L), "L_adv": float(La), "R": float(Rg),
           "grad": a.host(a.g).reshape(a.N, d)}
    if adv:
        got.update({"gamma": a.area("gamma", np.float32, ns * d).reshape(ns, d), "norm": a.area("norm", np.float32, ns),
                    "delta": a.area("delta", np.float32, ns * d).reshape(ns, d), "slot_of": a.area("slot_of", np.int32, 3 * nb),
                    "x_adv": a.area("x_adv", np.float32, nb), "c_adv": a.area("c_adv", np.float32, nb)})
    return got


def _check_plan(a, pl):
    ns = len(pl["rows"])
    run = a.area("run", np.int32, ns + 2)
    assert run[0] == ns and np.array_equal(run[1:], pl["starts"]), "the run table"
    assert np.array_equal(a.area("keys", np.uint64, 3 * a.n), pl["keys"]), "the sorted keys"


def _check_step(a, got, pl, lam, eps, adv_reg, prefix):
    tab = a.c["tab"]
    u, i, j = a.triplets()
    _report(R.check_chain(tab, u, i, j, a.U, lam, eps, adv_reg, got), prefix=prefix)
    if adv_reg != 0:
        want = R.walk_gamma32(tab, u, i, j, a.U, got["c"], pl)
        assert np.array_equal(R.bits(got["gamma"]), R.bits(want)), "Gamma is not the walk's bits"
        zero = ~got["gamma"].any(axis=1)
        assert not R.bits(got["delta"][zero]).any() and not R.bits(got["norm"][zero]).any(), "a zero row of Gamma: exact +0.0"
    want = R.walk_grad32(tab, u, i, j, a.U, got["c"], got.get("c_adv"), got.get("delta"), pl, lam, adv_reg)
    assert np.array_equal(R.bits(got["grad"]), R.bits(want)), "the gradient is not the walk's bits"


def _oracle_adam(p, g, m, v, t, lr=LR):
    p, m, v = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1).copy() for a in (p, m, v))
    orc.adam(p, np.ascontiguousarray(g, dtype=np.float32).reshape(-1), m, v, t, lr, B1, B2, ADAM_EPS)
    return p, m, v


def _check_adam(a, g, t, lr=LR, m0=None, v0=None):
    want = _oracle_adam(a.c["tab"], g, a.host_m if m0 is None else m0, a.host_v if v0 is None else v0, t, lr)
    for name, got, ref in zip("pmv", (a.host(a.tab), a.host(a.m), a.host(a.v)), want):
        assert np.array_equal(R.bits(got), R.bits(ref)), f"Adam: {name} is not the oracle's bits"


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_apr_step_stage_by_stage(gpu_device, case):
    c = R.named_case(*case)
    pl = c["ref"]["plan"]
    adam_t0 = (0, 2, 999)[R.CASES.index(case) % 3]
    a = Apr(gpu_device, c, state_seed=3)
    assert a.run(adam_t0=adam_t0) == 0, _lib.lib().rk_last_error()
    assert a.guards_intact() and a.host(a.status).view(np.int32).tolist() == [0, -1]
    _check_plan(a, pl)
    got = _stages(a, pl)
    assert np.all(a.words_outside(_written(a, len(pl["rows"]))) == SENT_BITS), "a word outside the stages' areas was written"
    _check_step(a, got, pl, c["lam"], c["eps"], c["adv_reg"], prefix=f"{IDS[R.CASES.index(case)]}.")
    _check_adam(a, got["grad"], adam_t0 + 1)
    assert not a.area("grad", np.uint32, a.N * a.d).any(), "the dense gradient buffer is not +0.0 after the Adam pass"


@pytest.mark.parametrize("adam_t0", [0, 2, 999])
def test_apr_adam_step_numbering(gpu_device, adam_t0):
    c = R.named_case(65, 200, "hubs")
    a = Apr(gpu_device, c, state_seed=4)
    assert a.run(adam_t0=adam_t0) == 0, _lib.lib().rk_last_error()
    _check_adam(a, a.host(a.g), adam_t0 + 1)


def test_apr_epoch_short_last_step_and_adam_numbering(gpu_device):
    """200 triplets in steps of 80: 80, 80, 40, with lr = 1e-3, so the tables move and Adam's t matters (it enters the step size and
    the bias correction).  The oracle is chained: step s is run on its own, without an update, on the table the ORACLE produced
    after step s - 1 -- every stage checked there, the short step dividing by 40 --, and orc.adam is applied to that gradient at
    t0 + s + 1.  After three steps the epoch's p, m and v equal the chain's bit for bit, and its loss rows the single steps'."""
    c, t0, B = R.named_case(64, 200, "hubs"), 5, 80
    a = Apr(gpu_device, c, batch=B, state_seed=6)
    assert a.run(adam_t0=t0) == 0, _lib.lib().rk_last_error()
    assert a.guards_intact() and a.lay.n_steps == 3 and a.lay.run_stride == 3 * B + 2
    rows = a.step_losses()
    tab, want_m, want_v = np.asarray(c["tab"], dtype=np.float32).reshape(-1), a.host_m, a.host_v
    for s, (lo, hi) in enumerate(((0, 80), (80, 160), (160, 200))):
        cs = dict(c, tab=tab.reshape(a.N, a.d).copy())
        one = Apr(gpu_device, cs, n=hi - lo, lo=lo)
        assert one.run(adam_t0=t0 + s, apply=0) == 0, _lib.lib().rk_last_error()
        u, i, j = one.triplets()
        pl = R.plan(u, i, j, c["U"])
        _check_plan(one, pl)
        got = _stages(one, pl)
        _check_step(one, got, pl, c["lam"], c["eps"], c["adv_reg"], prefix=f"epoch.step{s}.")
        assert np.array_equal(rows[s].view(np.uint64), one.step_losses()[0].view(np.uint64)), f"loss row {s} differs from the step on its own"
        run = a.area("run", np.int32, 3 * a.lay.run_stride)[s * a.lay.run_stride:][:len(pl["rows"]) + 2]
        assert run[0] == len(pl["rows"]) and np.array_equal(run[1:], pl["starts"])
        assert not _same(_oracle_adam(tab, got["grad"], want_m, want_v, t0 + s + 2)[0], _oracle_adam(tab, got["grad"], want_m, want_v, t0 + s + 1)[0]), \
            "t must matter to this check"
        tab, want_m, want_v = _oracle_adam(tab, got["grad"], want_m, want_v, t0 + s + 1)
    assert _same(a.host(a.g), got["grad"]), "desc.grad holds the last step's gradient"
    assert not _same(tab, c["tab"]) and _same(a.host(a.tab), tab), "p after three steps is not the chained oracle's"
    assert _same(a.host(a.m), want_m) and _same(a.host(a.v), want_v)
    assert not a.area("grad", np.uint32, a.N * a.d).any(), "the dense gradient buffer is not +0.0 after the epoch"


def test_apr_lr_0_moves_the_moments_only(gpu_device):
    c = R.named_case(17, 200, "hubs")
    a = Apr(gpu_device, c, state_seed=9)
    assert a.run(adam_t0=2, lr=0.0) == 0, _lib.lib().rk_last_error()
    assert a.guards_intact() and _same(a.host(a.tab), c["tab"]), "lr = 0 moved a parameter"
    _, want_m, want_v = _oracle_adam(c["tab"], a.host(a.g), a.host_m, a.host_v, 3, lr=0.0)
    assert _same(a.host(a.m), want_m) and _same(a.host(a.v), want_v) and not _same(want_m, a.host_m)


def test_apr_apply_update_0_leaves_tables_and_moments(gpu_device):
    c = R.named_case(17, 200, "hubs")
    a = Apr(gpu_device, c, state_seed=7)
    assert a.run(apply=0) == 0, _lib.lib().rk_last_error()
    for t, h in ((a.tab, c["tab"]), (a.m, a.host_m), (a.v, a.host_v)):
        assert _same(a.host(t), h), "apply_update = 0 moved a table or a moment"
    b = Apr(gpu_device, c, state_seed=7)
    assert b.run(apply=1) == 0
    assert np.array_equal(R.bits(a.host(a.g)), R.bits(b.host(b.g))) and a.host(a.g).any()
    assert not a.area("grad", np.uint32, a.N * a.d).any()
    nog = Apr(gpu_device, c, state_seed=7)
    assert nog.run(apply=1, grad=None) == 0, "desc.grad is optional with apply_update = 1"
    assert np.array_equal(R.bits(nog.host(nog.tab)), R.bits(b.host(b.tab))) and np.all(nog.host(nog.g).view(np.uint32) == SENT_BITS)


@pytest.mark.parametrize("case", [(64, 200, "hubs"), (3, 65, "plain"), (255, 200, "hubs")])
def test_apr_adv_reg_0_is_bpr_and_skips_steps_2_to_4(gpu_device, case):
    c = R.named_case(*case)
    pl = c["ref"]["plan"]
    a = Apr(gpu_device, c)
    assert a.run(adv_reg=0.0) == 0, _lib.lib().rk_last_error()
    for name, words in zip(STEP_AREAS, (3 * a.n, 3 * a.n * a.d, 3 * a.n, 3 * a.n * a.d, a.n, a.n)):
        assert np.all(a.area(name, np.uint32, words) == SENT_BITS), f"adv_reg = 0 wrote into {name}"
    assert np.all(a.words_outside(_written(a, len(pl["rows"]), adv=False)) == SENT_BITS)
    got = _stages(a, pl, adv=False)
    assert got["L_adv"] == 0.0
    _check_step(a, got, pl, c["lam"], c["eps"], 0.0, prefix="adv0.")
    _check_adam(a, got["grad"], 1)


def test_apr_eps_0_gives_delta_0_and_the_same_loss(gpu_device):
    c = R.named_case(64, 200, "hubs")
    pl = c["ref"]["plan"]
    a = Apr(gpu_device, c)
    assert a.run(eps=0.0) == 0, _lib.lib().rk_last_error()
    got = _stages(a, pl)
    assert not (got["delta"] != 0).any() and np.array_equal(R.bits(got["x_adv"]), R.bits(got["x"])) and np.array_equal(R.bits(got["c_adv"]), R.bits(got["c"]))
    assert got["L_adv"] == got["L"]
    _check_step(a, got, pl, c["lam"], 0.0, c["adv_reg"], prefix="eps0.")


@pytest.mark.parametrize("case", [(64, 1100, "hubs"), (17, 200, "one_user")])
def test_apr_same_call_twice_same_bits(gpu_device, case):
    c = R.named_case(*case)
    runs = []
    for _ in range(2):
        a = Apr(gpu_device, c, batch=96, state_seed=8)
        assert a.run(adam_t0=1) == 0, _lib.lib().rk_last_error()
        ws = a.words_outside({})                     # everything but the sort's own scratch and input
        runs.append([ws] + [a.host(t).view(np.uint32) for t in (a.tab, a.m, a.v, a.g, a.losses)])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


def _untouched(a):
    c = a.c
    assert a.guards_intact()
    assert np.all(a.ws.cpu().numpy().view(np.uint32) == SENT_BITS), "the workspace was written"
    assert np.all(a.host(a.losses).view(np.uint32) == SENT_BITS) and np.all(a.host(a.g).view(np.uint32) == SENT_BITS)
    for t, h in ((a.tab, c["tab"]), (a.m, a.host_m), (a.v, a.host_v)):
        assert _same(a.host(t), h)


def test_apr_refusals_launch_nothing(gpu_device):
    c = R.named_case(16, 65, "plain")
    nan, inf = float("nan"), float("inf")
    for what, kw in (("dim = 0", dict(dim=0)), ("dim = 257", dict(dim=257)), ("batch = 0", dict(batch=0)), ("batch = 65537", dict(batch=65537)),
                     ("n = 0", dict(n=0)), ("n < 0", dict(n=-3)), ("eps < 0", dict(eps=-0.5)), ("eps nan", dict(eps=nan)), ("eps inf", dict(eps=inf)),
                     ("adv_reg < 0", dict(adv_reg=-1.0)), ("adv_reg nan", dict(adv_reg=nan)), ("adv_reg inf", dict(adv_reg=inf)),
                     ("a small workspace", dict(workspace_bytes=None)), ("no workspace", dict(workspace=None)), ("no table", dict(table=None)),
                     ("no m", dict(m=None)), ("no v", dict(v=None)), ("no users", dict(users=None)), ("no pos", dict(pos=None)),
                     ("no neg", dict(neg=None)), ("no losses", dict(losses=None)), ("no status", dict(status=None)), ("no desc", dict(desc=False)),
                     ("n_users = 0", dict(n_users=0)), ("n_items = 0", dict(n_items=0)),
                     ("adam_t0 < 0", dict(adam_t0=-1)), ("a workspace off the 256-byte grid", dict(workspace="off")),
                     ("apply_update = 0 without grad", dict(grad=None, apply=0))):
        a = Apr(gpu_device, c)
        if "workspace_bytes" in kw:
            kw = dict(workspace_bytes=a.lay.bytes - 1)
        off = None
        if kw.get("workspace") == "off":
            off = torch.full((a.lay.bytes // 4 + 128,), R.SENTINEL, device=gpu_device, dtype=torch.float32)      # large enough, entered 4 bytes in
            kw = dict(workspace=off[1:], workspace_bytes=a.lay.bytes + 256)
        assert a.run(**kw) == EINVAL and _lib.lib().rk_last_error(), what
        _untouched(a)
        assert np.all(a.host(a.status).view(np.uint32) == SENT_BITS), what
        assert off is None or np.all(off.cpu().numpy().view(np.uint32) == SENT_BITS), what
    lay = _lib.AprLayout()
    for args in ((0, 70, 16, 65, 65), (40, 70, 0, 65, 65), (40, 70, 257, 65, 65), (40, 70, 16, 0, 65), (40, 70, 16, 65, 0), (40, 70, 16, 65, 65537),
                 (1 << 23, 1 << 23, 16, 65, 65), (40, 70, 16, 1 << 21, 1), (40, 70, 16, (1 << 31) // 3, 65536)):
        assert _lib.lib().rk_apr_workspace(*args, C.byref(lay)) == EINVAL, args
    assert _lib.lib().rk_apr_workspace(40, 70, 16, 65, 65, None) == EINVAL
    a = Apr(gpu_device, c)
    assert a.run() == 0


@pytest.mark.parametrize("col,t,value,rule", [(0, 7, 40, 9), (0, 64, -1, 9), (1, 0, 70, 10), (1, 33, -(1 << 40), 10), (2, 64, 70, 11),
                                               (2, 5, 1 << 40, 11)])
def test_apr_a_bad_id_is_refused_by_the_check_kernel_alone(gpu_device, col, t, value, rule):
    c = dict(R.named_case(16, 65, "plain"))
    key = "uij"[col]
    c[key] = c[key].copy()
    c[key][t] = value
    if t < 64:
        c["j"] = c["j"].copy()
        c["j"][64] = 1 << 50                      # a later violation too: the lowest triplet is the one reported
    a = Apr(gpu_device, c)
    assert a.run() == EINVAL and b"rule" in _lib.lib().rk_last_error()
    assert a.host(a.status).view(np.int32).tolist() == [rule, t]
    _untouched(a)
