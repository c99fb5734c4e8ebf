"""GPU tests of the Mult-VAE victim's kernels (recad_amd/csrc/multvae.hip) through the rk_mvae_* entries: every case of the table
of tests/_multvae_restate.py as a one-step epoch, each stage read out of the workspace behind sentinel prefills and compared with
the restatement of THAT stage fed the device's own inputs -- the masks, the item-grouped view, c, a, pre1, the nine products, the
tanh backwards, the bias sums, gW1 (its +0.0 rows included) and Adam bit for bit; h1, h2, z, KL, lse, nll, the loss, dl, dmu and
dlogvar within their counted budgets; eps against the float64 Box-Muller -- then the epoch loop (a short last step, Adam's
numbering), the switches (apply_update = 0, lr = 0), repeatability, inference (rk_mvae_scores, rk_mvae_pair_scores) and the
refusals.  Each test prints "RATIO <stage> <worst err / bound>" before it asserts <= 1."""
import ctypes as C

import numpy as np
import pytest
import torch

from recad_amd import _lib

from . import _multvae_restate as R

pytestmark = pytest.mark.gpu
EINVAL = -22
GUARD = 64
SENT_BITS = np.float32(R.SENTINEL).view(np.uint32)
LR, B1, B2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8
IDS = [name for name, _ in R.CASES]
BH = ("a", "pre1", "h1", "pre2", "h2", "dh2", "dp2", "dh1", "dp1")


def _same(a, b):
    return np.array_equal(R.bits(a).reshape(-1), R.bits(b).reshape(-1))


def _report(r, prefix=""):
    for k, v in r.items():
        print(f"RATIO {prefix}{k} {v:.4f}")
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad


class Mv:
    """device buffers of one call, every one between two margins of GUARD sentinel words"""

    def __init__(self, dev, c, users=None, batch=None, nnz_cap=None, state_seed=None, ptr=None, col=None):
        self.dev, self.c = dev, c
        self.I, self.H, self.L, self.U = c["I"], c["H"], c["L"], c["U"]
        self.users = np.asarray(c["users"] if users is None else users, dtype=np.int32)
        self.n = len(self.users)
        self.batch = self.n if batch is None else batch
        self.n_steps = (self.n + self.batch - 1) // self.batch
        self.ptr = np.asarray(c["ptr"] if ptr is None else ptr, dtype=np.int32)
        self.col = np.asarray(c["col"] if col is None else col, dtype=np.int32)
        self.bufs = []
        self.P = R.n_params(self.I, self.H, self.L)
        rng = np.random.default_rng(0 if state_seed is None else state_seed)
        self.host_m = (0.1 * rng.standard_normal(self.P)).astype(np.float32) if state_seed is not None else np.zeros(self.P, np.float32)
        self.host_v = (1e-3 * rng.random(self.P) + 1e-6).astype(np.float32) if state_seed is not None else np.zeros(self.P, np.float32)
        self.theta, self.m, self.v, self.g = self._buf(self.P, c["theta"]), self._buf(self.P, self.host_m), self._buf(self.P, self.host_v), self._buf(self.P)
        self.losses = self._buf(2 * 3 * self.n_steps)                      # doubles, as pairs of sentinel words
        self.status = self._buf(2)
        self.logits_out = self._buf(self.batch * self.I)
        self.ids = torch.from_numpy(self.users.copy()).to(dev)
        self.d_ptr, self.d_col = torch.from_numpy(self.ptr.copy()).to(dev), torch.from_numpy(self.col.copy()).to(dev)
        lens = np.diff(self.ptr)[np.clip(self.users, 0, self.U - 1)]
        per_step = [int(lens[s:s + self.batch].sum()) for s in range(0, self.n, self.batch)]
        self.nnz_cap = max(1, max(per_step)) if nnz_cap is None else nnz_cap
        self.lay = _lib.MvaeLayout()
        rc = _lib.lib().rk_mvae_workspace(self.I, self.H, self.L, self.batch, self.nnz_cap, C.byref(self.lay))
        assert rc == 0, _lib.lib().rk_last_error()
        assert self.lay.bytes % 256 == 0 and all(getattr(self.lay, k) % 256 == 0 for k in _lib.MvaeLayout.AREAS)
        self.ws = self._buf(self.lay.bytes // 4)
        assert self.ws.data_ptr() % 256 == 0
        self._raw = None

    def _buf(self, n, init=None):
        whole = torch.full((n + 2 * GUARD,), R.SENTINEL, device=self.dev, dtype=torch.float32)
        if init is not None:
            whole[GUARD:GUARD + n].copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32).reshape(-1)))
        self.bufs.append((whole, n))
        return whole[GUARD:GUARD + n]

    def guards_intact(self):
        return all(bool(np.all(np.r_[w[:GUARD].cpu().numpy(), w[GUARD + n:].cpu().numpy()].view(np.uint32) == SENT_BITS)) for w, n in self.bufs)

    def desc(self, lr=LR, **over):
        c = self.c
        a = dict(n_users=self.U, n_items=self.I, hidden=self.H, latent=self.L, rowptr=self.d_ptr, col=self.d_col, params=self.theta, m=self.m,
                 v=self.v, grad=self.g, logits_out=self.logits_out, dropout=c["dropout"], anneal_cap=c["cap"], total_anneal_steps=c["total"],
                 seed=c["seed"], ws_nnz_cap=self.nnz_cap, ws_batch=self.batch, workspace=self.ws, workspace_bytes=self.lay.bytes)
        a.update(over)
        p = lambda t: t.data_ptr() if torch.is_tensor(t) else t
        return _lib.MvaeDesc(lr=lr, beta1=B1, beta2=B2, adam_eps=ADAM_EPS, **{k: p(v) for k, v in a.items()})

    def run(self, step0=None, apply=1, lr=LR, n=None, batch=None, ids=True, losses=True, status=True, **over):
        desc = self.desc(lr, **over)
        rc = _lib.lib().rk_mvae_train_epoch(C.byref(desc), _lib.ptr(self.ids) if ids else None, self.n if n is None else n,
                                            self.batch if batch is None else batch, self.c["step0"] if step0 is None else step0, apply,
                                            _lib.ptr(self.losses) if losses else None, _lib.ptr(self.status) if status else None,
                                            _lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        self._raw = None
        return rc

    # ---- reading
    def raw(self):
        if self._raw is None:
            self._raw = self.ws.cpu().numpy().view(np.uint8)
        return self._raw

    def area(self, name, dtype, count):
        o = getattr(self.lay, name)
        return self.raw()[o:o + count * np.dtype(dtype).itemsize].view(dtype).copy()

    def words_outside(self, written):
        """the workspace's 32-bit words with the byte ranges of `written` ({area: bytes}) blanked to the sentinel: all that remains
        must be the prefill"""
        raw = self.raw().view(np.uint32).copy()
        for name, nbytes in written.items():
            o = getattr(self.lay, name)
            raw[o // 4:(o + nbytes + 3) // 4] = SENT_BITS
        return raw

    def step_losses(self):
        return self.losses.cpu().numpy().view(np.float64).reshape(self.n_steps, 3)

    def host(self, t):
        return t.cpu().numpy()

    def status_host(self):
        return self.status.cpu().numpy().view(np.int32).tolist()


def _written(a, nb, nnz):
    """bytes of each area a ONE-step training call writes"""
    I, H, L = a.I, a.H, a.L
    w = {"brp": 4 * (nb + 1), "keep": 4 * nnz, "keys": 8 * nnz, "keys_in": 8 * nnz, "t_ptr": 4 * (I + 1), "t_row": 4 * nnz, "c": 4 * nb,
         "ml": 8 * nb * L, "dml": 8 * nb * L, "eps": 4 * nb * L, "z": 4 * nb * L, "dz": 4 * nb * L, "kl": 8 * nb, "lse": 8 * nb, "nll": 8 * nb,
         "logits": 4 * nb * I, "grad": 4 * a.P}
    w.update({k: 4 * nb * H for k in BH})
    return w


def _stages(a, nb, nnz):
    """what a call whose last step had nb rows and nnz entries left in the workspace"""
    I, H, L = a.I, a.H, a.L
    f = np.float32
    got = {k: a.area(k, f, nb * H).reshape(nb, H) for k in BH}
    got.update({"brp": a.area("brp", np.int32, nb + 1), "keep": a.area("keep", np.int32, nnz), "t_ptr": a.area("t_ptr", np.int32, I + 1),
                "t_row": a.area("t_row", np.int32, nnz), "c": a.area("c", f, nb), "ml": a.area("ml", f, nb * 2 * L).reshape(nb, 2 * L),
                "dml": a.area("dml", f, nb * 2 * L).reshape(nb, 2 * L), "eps": a.area("eps", f, nb * L).reshape(nb, L),
                "z": a.area("z", f, nb * L).reshape(nb, L), "dz": a.area("dz", f, nb * L).reshape(nb, L), "kl": a.area("kl", np.float64, nb),
                "lse": a.area("lse", np.float64, nb), "nll": a.area("nll", np.float64, nb), "dl": a.area("logits", f, nb * I).reshape(nb, I),
                "logits": a.host(a.logits_out)[:nb * I].reshape(nb, I), "grad": a.area("grad", f, a.P)})
    return got


def _check_step(a, got, P, users, step, prefix="", b_div=None):
    """every stage of `got` against the restatement of that stage from got's own inputs; returns the masks"""
    c, I, L = a.c, a.I, a.L
    rows = [a.col[a.ptr[u]:a.ptr[u + 1]].astype(np.int64) for u in users]
    nb = len(users)
    beta = R.beta_at(step, c["cap"], c["total"])
    # the integer stages, exactly
    masks = R.keep_masks(c["seed"], step, users, rows, c["dropout"])
    assert np.array_equal(got["brp"], np.r_[0, np.cumsum([len(r) for r in rows])]), "brp"
    assert np.array_equal(got["keep"], np.concatenate(masks).astype(np.int32)), "the keep masks"
    kept = sorted((int(i), b) for b, (r, m) in enumerate(zip(rows, masks)) for i in r[m])
    want_ptr = np.searchsorted(np.array([i for i, _ in kept], dtype=np.int64), np.arange(I + 1))
    assert np.array_equal(got["t_ptr"], want_ptr) and np.array_equal(got["t_row"][:len(kept)], [b for _, b in kept]), "the item-grouped view"
    # bit for bit
    assert _same(got["c"], R.c_of([len(r) for r in rows], c["dropout"])), "c"
    assert _same(got["a"], R.a_walk(P["W1"], rows, masks)), "a"
    assert _same(got["pre1"], R.pre1_walk(got["c"], got["a"], P["b1"])), "pre1"
    assert _same(got["ml"], R.chain(got["h1"], P["W2"], P["b2"])), "ml"
    assert _same(got["pre2"], R.chain(got["z"], P["W3"], P["b3"])), "pre2"
    assert _same(got["logits"], R.chain(got["h2"], P["W4"], P["b4"])), "logits"
    assert _same(got["dh2"], R.chain(got["dl"], P["W4"].T)), "dh2"
    assert _same(got["dp2"], R.tanh_bwd_walk(got["dh2"], got["h2"])), "dp2"
    assert _same(got["dz"], R.chain(got["dp2"], P["W3"].T)), "dz"
    assert _same(got["dh1"], R.chain(got["dml"], P["W2"].T)), "dh1"
    assert _same(got["dp1"], R.tanh_bwd_walk(got["dh1"], got["h1"])), "dp1"
    want_grad = R.split(R.grads_walk(P, got, rows, masks, I), I, a.H, L)
    got_grad = R.split(got["grad"], I, a.H, L)
    for name in R.NAMES:
        assert _same(got_grad[name], want_grad[name]), f"g{name}"
    # eps against the float64 Box-Muller, then the tolerant stages
    e64 = R.eps64(c["seed"], step, users, L)
    r = {"eps": R.ratio(got["eps"], e64, 2.0 ** -23 * np.maximum(1.0, np.abs(e64)))}
    r.update(R.tolerant_ratios(got, P, rows, got["eps"], beta, b_div=b_div))
    _report(r, prefix)
    return masks


# ------------------------------------------------------------------------------------------------------ every case, stage by stage
@pytest.mark.parametrize("k", range(len(R.CASES)), ids=IDS)
def test_one_step_stage_by_stage(gpu_device, k):
    c = R.make_case(k)
    a = Mv(gpu_device, c)
    theta0 = c["theta"].copy()
    P = R.split(theta0, c["I"], c["H"], c["L"])
    assert a.run() == 0, _lib.lib().rk_last_error()
    assert a.status_host() == [0, -1]
    nb, nnz = a.n, int(np.diff(c["ptr"])[c["users"]].sum())
    got = _stages(a, nb, nnz)
    got["loss"] = a.step_losses()[0, 0]
    masks = _check_step(a, got, P, c["users"], c["step0"], prefix=f"{c['name']} ")
    loss, nll, kl = a.step_losses()[0]
    assert abs(nll - got["nll"].sum() / nb) <= 1e-12 * abs(nll) + 1e-300 and abs(kl - got["kl"].sum() / nb) <= 1e-12 * abs(kl) + 1e-300
    if c["B"] > 2:                       # the repeated user draws the same mask and the same noise in both positions
        assert _same(got["eps"][-1], got["eps"][0]) and np.array_equal(masks[-1], masks[0])
    untouched = np.diff(got["t_ptr"]) == 0
    assert np.all(R.bits(R.split(got["grad"], c["I"], c["H"], c["L"])["W1"][untouched]) == 0), "+0.0 rows of gW1"
    if c["special"] == "all_dropped":
        had = np.zeros(c["I"], bool)
        had[np.concatenate(c["rows"])] = True
        assert (had & untouched).any()
    # Adam, bit for bit against the oracle's
    want, m, v = theta0.copy(), a.host_m.copy(), a.host_v.copy()
    R.adam_oracle(want, got["grad"], m, v, c["step0"] + 1, LR, B1, B2, ADAM_EPS)
    assert _same(a.host(a.theta), want) and _same(a.host(a.m), m) and _same(a.host(a.v), v), "Adam"
    assert np.all(a.host(a.g).view(np.uint32) == SENT_BITS), "desc.grad is written with apply_update = 0 only"
    assert a.guards_intact()
    assert np.all(a.words_outside(_written(a, nb, nnz)) == SENT_BITS), "a word outside the step's areas was written"


@pytest.mark.parametrize("t0", [0, 2, 999])
def test_adam_numbering_from_a_warm_state(gpu_device, t0):
    c = R.make_case(10)
    a = Mv(gpu_device, c, state_seed=3)
    assert a.run(step0=t0) == 0, _lib.lib().rk_last_error()
    grad = a.area("grad", np.float32, a.P)
    want, m, v = c["theta"].copy(), a.host_m.copy(), a.host_v.copy()
    R.adam_oracle(want, grad, m, v, t0 + 1, LR, B1, B2, ADAM_EPS)
    assert _same(a.host(a.theta), want) and _same(a.host(a.m), m) and _same(a.host(a.v), v)
    assert not _same(want, c["theta"])


# ------------------------------------------------------------------------------------------------------ the noise
def test_eps_statistics_and_no_repeats_between_steps(gpu_device):
    c = R.make_case(12)                                  # B = 200, L = 33
    users = np.arange(200, dtype=np.int32)               # distinct users: 6600 independent draws
    draws = []
    for step in (c["step0"], c["step0"] + 1):
        a = Mv(gpu_device, c, users=users)
        assert a.run(step0=step, apply=0) == 0, _lib.lib().rk_last_error()
        draws.append(a.area("eps", np.float32, 200 * 33).astype(np.float64))
    e, n = draws[0], 6600
    print(f"EPS mean {e.mean():+.4f} (sigma {n ** -0.5:.4f}), variance {e.var():.4f} (sigma {(2 / n) ** 0.5:.4f})")
    assert abs(e.mean()) <= 5 * n ** -0.5 and abs(e.var() - 1.0) <= 5 * (2.0 / n) ** 0.5
    # a stuck counter would repeat a position's value in the next step; two of 6600 fp32 normals coincide by chance 0.65 times
    # on average (2.2e7 pairs, a density of 0.3 over a spacing of 1e-7), so a few equal values inside a draw mean nothing
    assert not np.any(draws[0] == draws[1]) and len(np.unique(e)) >= n - 3


# ------------------------------------------------------------------------------------------------------ the epoch loop
def test_three_steps_with_a_short_last_one(gpu_device):
    c = R.make_case(10)                                  # 200 users in steps of 80, 80, 40
    users = c["users"]
    whole = Mv(gpu_device, c, batch=80)
    assert whole.run() == 0, _lib.lib().rk_last_error()
    two = Mv(gpu_device, c, users=users[:160], batch=80, nnz_cap=whole.nnz_cap)
    assert two.run() == 0, _lib.lib().rk_last_error()
    assert np.array_equal(whole.step_losses()[:2], two.step_losses())
    # the last step from the state the two-step epoch left: every stage, then the oracle's Adam at t = step0 + 3
    theta2 = two.host(two.theta).copy()
    P = R.split(theta2, c["I"], c["H"], c["L"])
    last = users[160:]
    nnz = int(np.diff(c["ptr"])[last].sum())
    got = _stages(whole, 40, nnz)
    got["loss"] = whole.step_losses()[2, 0]
    _check_step(whole, got, P, last, c["step0"] + 2, prefix="short ", b_div=40)
    m, v = two.host(two.m).copy(), two.host(two.v).copy()
    R.adam_oracle(theta2, got["grad"], m, v, c["step0"] + 3, LR, B1, B2, ADAM_EPS)
    assert _same(whole.host(whole.theta), theta2) and _same(whole.host(whole.m), m) and _same(whole.host(whole.v), v)
    assert whole.guards_intact() and two.guards_intact()


def test_apply_update_0_and_lr_0(gpu_device):
    c = R.make_case(11)
    a = Mv(gpu_device, c, state_seed=4)
    assert a.run(apply=0) == 0, _lib.lib().rk_last_error()
    assert _same(a.host(a.theta), c["theta"]) and _same(a.host(a.m), a.host_m) and _same(a.host(a.v), a.host_v)
    grad = a.area("grad", np.float32, a.P)
    assert _same(a.host(a.g), grad) and np.abs(grad).max() > 0
    b = Mv(gpu_device, c, state_seed=4)
    assert b.run(lr=0.0) == 0, _lib.lib().rk_last_error()
    assert _same(b.host(b.theta), c["theta"]) and not _same(b.host(b.m), b.host_m) and not _same(b.host(b.v), b.host_v)
    assert np.array_equal(a.step_losses(), b.step_losses())
    assert a.run(apply=0, grad=None) == EINVAL


def test_the_same_call_twice_gives_the_same_bits(gpu_device):
    c = R.make_case(12)
    out = []
    for _ in range(2):
        a = Mv(gpu_device, c, batch=80)
        assert a.run() == 0, _lib.lib().rk_last_error()
        out.append((a.host(a.theta).copy(), a.host(a.m).copy(), a.host(a.v).copy(), a.step_losses().copy(), a.area("grad", np.float32, a.P),
                    a.area("logits", np.float32, 40 * c["I"])))
    for x, y in zip(*out):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ------------------------------------------------------------------------------------------------------ inference
def _scores(a, users, ws_batch=None, **over):
    ids = torch.from_numpy(np.asarray(users, dtype=np.int32)).to(a.dev)
    out = a._buf(len(users) * a.I)
    desc = a.desc(m=None, v=None, grad=None, logits_out=None, **over)
    rc = _lib.lib().rk_mvae_scores(C.byref(desc), _lib.ptr(ids), len(users), _lib.ptr(out), a.I, _lib.stream_ptr(a.dev))
    torch.cuda.synchronize()
    a._raw = None
    return rc, out


@pytest.mark.parametrize("k", [1, 6, 10, 12, 13, 17, 20], ids=lambda k: IDS[k])
def test_scores_against_the_inference_restatement(gpu_device, k):
    c = R.make_case(k)
    a = Mv(gpu_device, c)
    users = np.r_[c["users"], c["U"] - 1][:a.batch]              # a user outside the training batch among them
    rc, out = _scores(a, users)
    assert rc == 0, _lib.lib().rk_last_error()
    nb, I, H, L = len(users), c["I"], c["H"], c["L"]
    P = R.split(c["theta"], I, H, L)
    rows = [c["col"][c["ptr"][u]:c["ptr"][u + 1]].astype(np.int64) for u in users]
    every = [np.ones(len(r), bool) for r in rows]
    got = {k_: a.area(k_, np.float32, nb * H).reshape(nb, H) for k_ in ("a", "pre1", "h1", "pre2", "h2")}
    mu = a.area("ml", np.float32, nb * L).reshape(nb, L)
    S = a.host(out).reshape(nb, I)
    assert _same(a.area("c", np.float32, nb), R.c_of([len(r) for r in rows], 0.0)), "no dropout at inference"
    assert _same(got["a"], R.a_walk(P["W1"], rows, every)) and _same(got["pre1"], R.pre1_walk(a.area("c", np.float32, nb), got["a"], P["b1"]))
    assert _same(mu, R.chain(got["h1"], P["W2"][:L], P["b2"][:L])), "only the first L rows of W2"
    assert _same(got["pre2"], R.chain(mu, P["W3"], P["b3"])), "z = mu"
    assert _same(S, R.chain(got["h2"], P["W4"], P["b4"]))
    _report({"h1": R.ratio(got["h1"], R.st_tanh(got["pre1"]), R.bud_tanh(got["pre1"])),
             "h2": R.ratio(got["h2"], R.st_tanh(got["pre2"]), R.bud_tanh(got["pre2"]))}, prefix=f"scores {c['name']} ")
    want = R.step({n: v.astype(np.float64) for n, v in P.items()}, rows, None, None, 0.0, 0.0, train=False)["logits"]
    assert np.abs(S - want).max() <= 2.0 ** -12 * max(1.0, np.abs(want).max()), "the float64 inference end to end"
    assert _same(a.host(a.theta), c["theta"]) and a.guards_intact()


def test_scores_in_blocks_and_500_pairs_equal_the_matrix(gpu_device):
    c = R.make_case(11)                                           # I 300, H 65, L 33
    rng = np.random.default_rng(2)
    users = rng.integers(0, c["U"], 150).astype(np.int32)         # repeated users among them
    a = Mv(gpu_device, c, users=users)
    rc, out = _scores(a, users)
    assert rc == 0, _lib.lib().rk_last_error()
    S = a.host(out).reshape(150, c["I"]).copy()
    small = Mv(gpu_device, c, users=users[:64])                   # a workspace of 64 rows: three blocks
    rc, out2 = _scores(small, users)
    assert rc == 0, _lib.lib().rk_last_error()
    assert _same(small.host(out2), S) and small.guards_intact()
    assert _same(S[0], S[np.nonzero(users == users[0])[0][-1]])
    pu = rng.integers(0, 150, 500)
    pi = rng.integers(0, c["I"], 500).astype(np.int32)
    d_u, d_i = torch.from_numpy(users[pu].copy()).to(gpu_device), torch.from_numpy(pi).to(gpu_device)
    pairs = small._buf(500)
    desc = small.desc(m=None, v=None, grad=None, logits_out=None)
    rc = _lib.lib().rk_mvae_pair_scores(C.byref(desc), _lib.ptr(d_u), _lib.ptr(d_i), 500, _lib.ptr(pairs), _lib.stream_ptr(gpu_device))
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().rk_last_error()
    assert _same(small.host(pairs), S[pu, pi]), "a pair equals the matrix entry to the bit"
    assert _lib.lib().rk_mvae_pair_scores(C.byref(desc), None, None, 0, None, _lib.stream_ptr(gpu_device)) == 0
    d_i[7] = c["I"]
    assert _lib.lib().rk_mvae_pair_scores(C.byref(desc), _lib.ptr(d_u), _lib.ptr(d_i), 500, _lib.ptr(pairs), _lib.stream_ptr(gpu_device)) == EINVAL
    assert b"rule 16" in _lib.lib().rk_last_error()
    assert small.guards_intact()


# ------------------------------------------------------------------------------------------------------ the refusals
def _untouched(a, theta0):
    return (a.guards_intact() and np.all(a.host(a.ws).view(np.uint32) == SENT_BITS) and np.all(a.host(a.losses).view(np.uint32) == SENT_BITS)
            and _same(a.host(a.theta), theta0) and np.all(a.host(a.logits_out).view(np.uint32) == SENT_BITS))


def test_refusals_launch_nothing(gpu_device):
    c = R.make_case(11)
    a = Mv(gpu_device, c)
    for over in (dict(hidden=0), dict(hidden=1025), dict(latent=0), dict(latent=513), dict(ws_batch=0), dict(ws_batch=4097),
                 dict(workspace_bytes=a.lay.bytes - 1), dict(workspace=a.ws.data_ptr() + 4), dict(workspace=None), dict(params=None),
                 dict(m=None), dict(rowptr=None), dict(dropout=1.0), dict(dropout=-0.5), dict(anneal_cap=-1.0), dict(anneal_cap=float("inf")),
                 dict(total_anneal_steps=-1), dict(n_items=0), dict(ws_nnz_cap=0)):
        assert a.run(**over) == EINVAL, over
        assert _lib.lib().rk_last_error(), over
        assert _untouched(a, c["theta"]) and np.all(a.host(a.status).view(np.uint32) == SENT_BITS), over
    for kw in (dict(n=0), dict(batch=0), dict(batch=a.batch + 1), dict(step0=-1), dict(ids=False), dict(losses=False), dict(status=False)):
        assert a.run(**kw) == EINVAL, kw
        assert _untouched(a, c["theta"]), kw
    assert _lib.lib().rk_mvae_train_epoch(None, _lib.ptr(a.ids), a.n, a.batch, 0, 1, _lib.ptr(a.losses), _lib.ptr(a.status), None) == EINVAL
    rc, out = _scores(a, c["users"], hidden=1025)
    assert rc == EINVAL and np.all(a.host(out).view(np.uint32) == SENT_BITS)


def test_bad_ids_are_reported_by_the_check_kernel(gpu_device):
    c = R.make_case(11)                                           # B = 2 ... use a longer list of users
    c10 = R.make_case(10)
    for rule, make in ((12, "user_hi"), (12, "user_neg"), (13, "not_ascending"), (13, "item_hi"), (14, "empty"), (15, "cap")):
        users, ptr, col, nnz_cap = c10["users"].copy(), c10["ptr"].copy(), c10["col"].copy(), None
        at = 57
        if make == "user_hi":
            users[at] = c10["U"]
        elif make == "user_neg":
            users[at], users[at + 3] = -1, c10["U"] + 5           # the lowest position is reported
        elif make == "not_ascending":
            u = users[at]
            assert ptr[u + 1] - ptr[u] >= 2
            col[ptr[u] + 1] = col[ptr[u]]
        elif make == "item_hi":
            col[ptr[users[at] + 1] - 1] = c10["I"]
        elif make == "empty":
            u = users[at]
            cut = ptr[u + 1] - ptr[u]
            col = np.r_[col[:ptr[u]], col[ptr[u + 1]:]]
            ptr = ptr.copy()
            ptr[u + 1:] -= cut
        elif make == "cap":
            nnz_cap = int(np.diff(ptr)[users].sum()) - 1
        a = Mv(gpu_device, c10, users=users, ptr=ptr, col=col, nnz_cap=nnz_cap)
        assert a.run() == EINVAL, make
        where = 0 if make == "cap" else min(np.nonzero(users == users[at])[0][0], at) if make in ("not_ascending", "item_hi", "empty") else at
        assert a.status_host() == [rule, where], (make, a.status_host())
        assert f"rule {rule}".encode() in _lib.lib().rk_last_error()
        assert _untouched(a, c10["theta"]), make
    a = Mv(gpu_device, c)
    rc, out = _scores(a, np.array([0, c["U"]], dtype=np.int32))
    assert rc == EINVAL and b"rule 12" in _lib.lib().rk_last_error() and np.all(a.host(out).view(np.uint32) == SENT_BITS)
