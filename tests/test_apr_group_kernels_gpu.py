"""GPU tests of rk_apr_train_epoch_group (recad_amd/csrc/apr.hip): a group of APR models trained in shared launches.  The definition
is bit equality with rk_apr_train_epoch, so every case runs the group entry on one set of buffers and the SINGLE entry, member by
member, on copies of the same inputs (same sentinel prefills, same margins, same alignment of the table), and compares table,
moments, desc.grad, losses, status and the whole workspace but the radix sort's own input and scratch, margins included, word for
word.  No tolerance anywhere.  The reference side is always the single entry, which tests/test_apr_kernels_gpu.py pins to the numpy
walk and the oracle.  Then the refusals, each with nothing written."""
import ctypes as C

import numpy as np
import pytest
import torch

from recad_amd import _lib

from . import _apr_restate as R
from . import test_apr_kernels_gpu as K

pytestmark = pytest.mark.gpu
EINVAL, GUARD, SENT_BITS = K.EINVAL, K.GUARD, K.SENT_BITS
SIZES = ((40, 70), (47, 70), (33, 51))


def rand_case(U, I, d, n, seed, lam=R.LAM, eps=R.EPS, adv_reg=R.ADV_REG):
    """a drawn case in the form of _apr_restate.case: rows of norm about 1, i != j"""
    rng = np.random.default_rng(seed)
    tab = (rng.standard_normal((U + I, d)) / np.sqrt(d)).astype(np.float32)
    u, i = rng.integers(0, U, n), rng.integers(0, I, n)
    j = (i + 1 + rng.integers(0, I - 1, n)) % I
    return {"d": d, "U": U, "I": I, "tab": tab, "u": u.astype(np.int64), "i": i.astype(np.int64), "j": j.astype(np.int64), "lam": lam, "eps": eps,
            "adv_reg": adv_reg}


class Member(K.Apr):
    """the buffers of one member, with what the call is to be given for it.  shift: the table starts `shift` floats off its
    16-byte-aligned place"""

    def __init__(self, dev, c, n=None, batch=None, adam_t0=0, lr=K.LR, state_seed=None, shift=0, call_n=None, **over):
        super().__init__(dev, c, n=n, batch=batch, state_seed=state_seed)
        self.adam_t0, self.lr, self.over = adam_t0, lr, over
        if call_n is not None:                      # the n the call is given, the buffers being those of the case's own n
            over["n"] = call_n
        if shift:
            tot = self.N * self.d
            whole = torch.full((tot + 2 * GUARD + shift,), R.SENTINEL, device=dev, dtype=torch.float32)
            tab = whole[GUARD + shift:GUARD + shift + tot]
            tab.copy_(self.tab)
            self.bufs[0] = (whole[shift:], tot)
            self.tab = tab
        assert (self.tab.data_ptr() % 16 == 0) == (shift % 4 == 0)

    def args(self):
        c = self.c
        a = dict(n_users=self.U, n_items=self.I, dim=self.d, table=self.tab, m=self.m, v=self.v, grad=self.g, lam=c["lam"], eps=c["eps"],
                 adv_reg=c["adv_reg"], workspace=self.ws, workspace_bytes=self.lay.bytes, n=self.n, users=self.ids[0], pos=self.ids[1],
                 neg=self.ids[2], losses=self.losses, adam_t0=self.adam_t0)
        a.update(self.over)
        return a

    def single(self, batch, apply):
        over = {k: v for k, v in self.over.items() if k != "adam_t0"}
        return self.run(adam_t0=self.args()["adam_t0"], apply=apply, lr=self.lr, batch=batch, **over)

    def snapshot(self):
        """every word the call may write: the workspace but the sort's input and scratch, and all other buffers with their margins"""
        return [self.words_outside({})] + [w.cpu().numpy().view(np.uint32) for w, _ in self.bufs[:5]]

    def adv(self):
        return self.args()["adv_reg"] != 0


def _p(t):
    if t is None:
        return None
    return t if isinstance(t, int) else t.data_ptr()


class Group:
    def __init__(self, dev, members):
        self.dev, self.members, self.R = dev, members, len(members)
        self.whole = torch.full((2 * self.R + 2 * GUARD,), R.SENTINEL, device=dev, dtype=torch.float32)
        self.status = self.whole[GUARD:GUARD + 2 * self.R]

    def call(self, batch, apply=1, n_rep=None, missing=(), status=True):
        """missing: names among descs, users, pos, neg, n, adam_t0, losses -> a NULL array"""
        Rn = self.R
        a = [m.args() for m in self.members]
        descs = (_lib.AprDesc * Rn)()
        for r, (m, x) in enumerate(zip(self.members, a)):
            descs[r] = _lib.AprDesc(n_users=x["n_users"], n_items=x["n_items"], dim=x["dim"], table=_p(x["table"]), m=_p(x["m"]), v=_p(x["v"]),
                                    grad=_p(x["grad"]), lam=x["lam"], eps=x["eps"], adv_reg=x["adv_reg"], lr=m.lr, beta1=K.B1, beta2=K.B2,
                                    adam_eps=K.ADAM_EPS, workspace=_p(x["workspace"]), workspace_bytes=x["workspace_bytes"])
        arrays = {"descs": descs, "n": (C.c_int64 * Rn)(*[x["n"] for x in a]), "adam_t0": (C.c_int32 * Rn)(*[x["adam_t0"] for x in a])}
        for k in ("users", "pos", "neg", "losses"):
            arrays[k] = (C.c_void_p * Rn)(*[_p(x[k]) for x in a])
        for k in missing:
            arrays[k] = None
        rc = _lib.lib().rk_apr_train_epoch_group(Rn if n_rep is None else n_rep, arrays["descs"], arrays["users"], arrays["pos"], arrays["neg"],
                                                 arrays["n"], batch, arrays["adam_t0"], apply, arrays["losses"],
                                                 _lib.ptr(self.status) if status else None, _lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc

    def status_words(self):
        return self.status.cpu().numpy().view(np.int32).reshape(self.R, 2)

    def status_untouched(self):
        return bool(np.all(self.whole.cpu().numpy().view(np.uint32) == SENT_BITS))

    def margins_intact(self):
        w = self.whole.cpu().numpy().view(np.uint32)
        return bool(np.all(w[:GUARD] == SENT_BITS) and np.all(w[GUARD + 2 * self.R:] == SENT_BITS))


def run_pair(dev, specs, batch, apply=1, order=None):
    """specs: per member the keyword arguments of Member.  -> (the group's members, the single entry's) after both have run and every
    member's words have been found equal"""
    grouped = [Member(dev, batch=batch, **s) for s in specs]
    alone = [Member(dev, batch=batch, **s) for s in specs]
    order = list(range(len(specs))) if order is None else order
    g = Group(dev, [grouped[r] for r in order])
    assert g.call(batch, apply) == 0, _lib.lib().rk_last_error()
    assert g.margins_intact()
    status = g.status_words()
    for at, r in enumerate(order):
        assert alone[r].single(batch, apply) == 0, _lib.lib().rk_last_error()
        assert grouped[r].guards_intact() and alone[r].guards_intact()
        assert status[at].tolist() == alone[r].host(alone[r].status).view(np.int32).tolist() == [0, -1]
        for k, (x, y) in enumerate(zip(grouped[r].snapshot(), alone[r].snapshot())):
            assert np.array_equal(x, y), f"member {r}: buffer {k} (0 = workspace, then table, m, v, grad, losses) differs from the single entry's"
        a = grouped[r]
        assert not a.area("grad", np.uint32, a.N * a.d).any(), f"member {r}: the dense gradient buffer is not +0.0 after its epoch"
        if not a.adv():
            nb = min(batch, a.n)
            for name, words in zip(K.STEP_AREAS, (3 * nb, 3 * nb * a.d, 3 * nb, 3 * nb * a.d, nb, nb)):
                assert np.all(a.area(name, np.uint32, words) == SENT_BITS), f"member {r}: adv_reg = 0 wrote into {name}"
    return grouped, alone


def _moved(members):
    for a in members:
        assert not K._same(a.host(a.tab), a.c["tab"]), "the tables must move for the comparison to mean anything"


def _mixed_specs(Rn, d, batch, seed, sizes=SIZES):
    """Rn members of mixed sizes, triplet counts (so step counts), hyperparameters and Adam clocks"""
    ns = [n for n in (3 * batch + 7, batch, 1, batch + 1, batch - 1) if n >= 1]
    specs = []
    for r in range(Rn):
        U, I = sizes[r % len(sizes)]
        c = rand_case(U, I, d, ns[r % len(ns)], seed + r, lam=(0.01, 0.0, 0.1)[r % 3], eps=(0.5, 0.0)[(r // 2) % 2], adv_reg=(1.0, 0.0)[r % 2])
        specs.append(dict(c=c, adam_t0=(0, 2, 999)[r % 3], lr=(1e-3, 1e-2)[r % 2], state_seed=seed + 100 + r))
    return specs


@pytest.mark.parametrize("Rn", [1, 2, 3, 5, 16])
def test_group_sizes_mixed_members(gpu_device, Rn):
    """sizes (40, 70), (47, 70), (33, 51), n in {3 B + 7, B, 1, B + 1, B - 1} (4, 1, 1, 2 and 1 steps), adv_reg in {1, 0}, eps in
    {0.5, 0}, three lam, two lr and adam_t0 in {0, 2, 999} in one group"""
    specs = _mixed_specs(Rn, 16, 64, 1000 * Rn)
    grouped, _ = run_pair(gpu_device, specs, 64)
    _moved(grouped)
    if Rn >= 5:
        assert {a.n_steps for a in grouped} == {1, 2, 4} and {(a.U, a.I) for a in grouped} == set(SIZES)


def test_group_of_64_small_members(gpu_device):
    rng = np.random.default_rng(64)
    specs = [dict(c=rand_case(*SIZES[r % 3], 3, int(rng.integers(1, 11)), 6400 + r, adv_reg=float(r % 2)), adam_t0=r % 5, state_seed=r + 1)
             for r in range(64)]
    grouped, _ = run_pair(gpu_device, specs, 4)
    assert {a.n_steps for a in grouped} == {1, 2, 3}
    _moved(grouped)


@pytest.mark.parametrize("d", [1, 3, 16, 63, 64, 65, 128, 256])
def test_group_dims(gpu_device, d):
    grouped, _ = run_pair(gpu_device, _mixed_specs(3, d, 64, 77 * d), 64)
    _moved(grouped)
    assert all((a.tab.data_ptr() % 16) == 0 for a in grouped)


def test_group_d64_members_take_different_load_paths(gpu_device):
    """the middle member's table is 4 bytes off the 16-byte grid: it takes the scalar loads while its neighbours take float4,
    in the same launches, and each equals the single entry on a table placed the same way"""
    specs = _mixed_specs(3, 64, 64, 640)
    specs[1]["shift"] = 1
    grouped, alone = run_pair(gpu_device, specs, 64)
    assert [a.tab.data_ptr() % 16 for a in grouped] == [0, 4, 0] == [a.tab.data_ptr() % 16 for a in alone]
    _moved(grouped)


@pytest.mark.parametrize("batch", [1, 64, 200])
def test_group_batches_and_step_counts(gpu_device, batch):
    """n from {1, B - 1, B, B + 1, 3 B + 7}: members finish after 1, 2 and 4 steps in one group (1, 2 and 10 at B = 1).  A finished
    member's table, moments and zeroed gradient are those of its own last step (the single entry ran no further), although the group
    ran on: run_pair compares them and checks the gradient area for +0.0."""
    ns = sorted({max(1, n) for n in (1, batch - 1, batch, batch + 1, 3 * batch + 7)})
    specs = [dict(c=rand_case(*SIZES[r % 3], 16, n, 31 * batch + r, adv_reg=(0.5, 0.0)[r % 2]), adam_t0=r, state_seed=batch + r) for r, n in enumerate(ns)]
    grouped, _ = run_pair(gpu_device, specs, batch)
    assert {a.n_steps for a in grouped} == ({1, 2, 10} if batch == 1 else {1, 2, 4})
    _moved(grouped)


@pytest.mark.parametrize("adv", ["all_bpr", "all_adv"])
def test_group_all_bpr_and_all_adversarial(gpu_device, adv):
    specs = _mixed_specs(4, 16, 64, 4242)
    for r, s in enumerate(specs):
        s["adv_reg"] = 0.0 if adv == "all_bpr" else (0.5, 1.0)[r % 2]
    grouped, _ = run_pair(gpu_device, specs, 64)
    assert all(a.adv() == (adv == "all_adv") for a in grouped)
    _moved(grouped)


def test_group_apply_update_0_with_grad(gpu_device):
    specs = _mixed_specs(3, 16, 64, 909)
    grouped, _ = run_pair(gpu_device, specs, 64, apply=0)
    for a in grouped:
        assert K._same(a.host(a.tab), a.c["tab"]) and K._same(a.host(a.m), a.host_m) and a.host(a.g).any()


def test_group_lr_0_moves_the_moments_only(gpu_device):
    specs = _mixed_specs(3, 16, 64, 303)
    specs[1]["lr"] = 0.0
    grouped, _ = run_pair(gpu_device, specs, 64)
    a = grouped[1]
    assert K._same(a.host(a.tab), a.c["tab"]) and not K._same(a.host(a.m), a.host_m)
    _moved([grouped[0], grouped[2]])


@pytest.mark.parametrize("case", [(64, 200, "hubs"), (17, 200, "one_user"), (65, 200, "hubs")])
def test_group_hard_triplet_sets_next_to_an_easy_one(gpu_device, case):
    """the planted structures of tests/_apr_restate.py (runs of up to 200 incidences, the item that is positive and negative,
    x = +-40, a zero row; all triplets on one user: one run of 200) in one member, whose 200 triplets are one step, drawn sets of one
    and of three steps in the others"""
    d = case[0]
    hard = R.named_case(*case)
    specs = [dict(c=rand_case(47, 70, d, 90, 5, adv_reg=0.0), state_seed=1), dict(c=hard, state_seed=2, adam_t0=2),
             dict(c=rand_case(33, 51, d, 450, 6), state_seed=3)]
    grouped, _ = run_pair(gpu_device, specs, 200)
    assert [a.n_steps for a in grouped] == [1, 1, 3]
    assert int(grouped[1].area("run", np.int32, 2)[0]) == len(hard["ref"]["plan"]["rows"]), "the hard member's step is the planted batch"
    _moved(grouped)


def test_group_same_call_twice_and_member_order_reversed(gpu_device):
    specs = _mixed_specs(5, 64, 64, 2024)
    first, _ = run_pair(gpu_device, specs, 64)
    again = [Member(gpu_device, batch=64, **s) for s in specs]
    assert Group(gpu_device, again).call(64) == 0
    back, _ = run_pair(gpu_device, specs, 64, order=[4, 3, 2, 1, 0])
    for r in range(5):
        for x, y, z in zip(first[r].snapshot(), again[r].snapshot(), back[r].snapshot()):
            assert np.array_equal(x, y), f"member {r}: the same call twice"
            assert np.array_equal(x, z), f"member {r}: the member order reversed"


# ------------------------------------------------------------------------------------------------------------ refusals
def _three(dev, **middle):
    specs = [dict(c=rand_case(*SIZES[r], 16, 65, 50 + r), state_seed=r + 1) for r in range(3)]
    specs[1].update(middle)
    return [Member(dev, batch=65, **s) for s in specs]


def _nothing_written(g, what):
    for a in g.members:
        K._untouched(a)
    assert g.status_untouched(), what


def test_group_refusals_launch_nothing(gpu_device):
    nan, inf = float("nan"), float("inf")
    for what, kw in (("dim = 0", dict(dim=0)), ("dim = 257", dict(dim=257)), ("another dim", dict(dim=8)), ("n = 0", dict(call_n=0)), ("n < 0", dict(call_n=-3)),
                     ("eps < 0", dict(eps=-0.5)), ("eps nan", dict(eps=nan)), ("eps inf", dict(eps=inf)), ("adv_reg < 0", dict(adv_reg=-1.0)),
                     ("adv_reg nan", dict(adv_reg=nan)), ("adv_reg inf", dict(adv_reg=inf)), ("no workspace", dict(workspace=None)),
                     ("no table", dict(table=None)), ("no m", dict(m=None)), ("no v", dict(v=None)), ("no users", dict(users=None)),
                     ("no pos", dict(pos=None)), ("no neg", dict(neg=None)), ("no losses", dict(losses=None)), ("n_users = 0", dict(n_users=0)),
                     ("n_items = 0", dict(n_items=0)), ("adam_t0 < 0", dict(adam_t0=-1)), ("a small workspace", dict(workspace_bytes=256))):
        g = Group(gpu_device, _three(gpu_device, **kw))
        assert g.call(65) == EINVAL and _lib.lib().rk_last_error(), what
        _nothing_written(g, what)
    for what, kw in (("batch = 0", dict(batch=0)), ("batch = 65537", dict(batch=65537)), ("n_rep = 0", dict(batch=65, n_rep=0)),
                     ("n_rep = -1", dict(batch=65, n_rep=-1)), ("n_rep = 65", dict(batch=65, n_rep=_lib.RK_APR_MAX_GROUP + 1)),
                     ("no status", dict(batch=65, status=False))) + \
            tuple((f"no {k}", dict(batch=65, missing=(k,))) for k in ("descs", "users", "pos", "neg", "n", "adam_t0", "losses")):
        g = Group(gpu_device, _three(gpu_device))
        assert g.call(**kw) == EINVAL and _lib.lib().rk_last_error(), what
        _nothing_written(g, what)
    g = Group(gpu_device, _three(gpu_device, grad=None))
    assert g.call(65, apply=0) == EINVAL, "apply_update = 0 without grad"
    _nothing_written(g, "apply_update = 0 without grad")
    members = _three(gpu_device)
    off = torch.full((members[1].lay.bytes // 4 + 128,), R.SENTINEL, device=gpu_device, dtype=torch.float32)      # large enough, entered 4 bytes in
    members[1].over.update(workspace=off[1:], workspace_bytes=members[1].lay.bytes + 256)
    g = Group(gpu_device, members)
    assert g.call(65) == EINVAL, "a workspace off the 256-byte grid"
    _nothing_written(g, "a workspace off the 256-byte grid")
    assert np.all(off.cpu().numpy().view(np.uint32) == SENT_BITS)
    g = Group(gpu_device, _three(gpu_device))
    assert g.call(65) == 0 and g.status_words().tolist() == [[0, -1]] * 3


def test_group_overlapping_members_are_refused(gpu_device):
    for what in ("table", "m on table", "grad", "workspace", "the same member twice"):
        members = _three(gpu_device)
        a, b = members[0], members[2]
        if what == "table":                         # b's table starts inside a's (a has 110 rows, b 84)
            b.over.update(table=a.tab.data_ptr() + 4 * 16 * 30)
        elif what == "m on table":
            b.over.update(m=a.tab.data_ptr())
        elif what == "grad":
            b.over.update(grad=a.g.data_ptr() + 4)
        elif what == "workspace":                   # 256 bytes into a's workspace: aligned, and claimed to be long enough
            b.over.update(workspace=a.ws.data_ptr() + 256, workspace_bytes=b.lay.bytes)
        else:
            members[2] = members[0]
        g = Group(gpu_device, members)
        assert g.call(65) == EINVAL and b"share" in _lib.lib().rk_last_error(), what
        _nothing_written(g, what)


@pytest.mark.parametrize("col,t,value,rule", [(0, 7, 47, 9), (0, 64, -1, 9), (1, 0, 70, 10), (1, 33, -(1 << 40), 10), (2, 64, 70, 11), (2, 5, 1 << 40, 11)])
def test_group_a_bad_id_in_the_middle_member(gpu_device, col, t, value, rule):
    """the middle member has 47 users and 70 items"""
    c = dict(rand_case(*SIZES[1], 16, 65, 51))
    key = "uij"[col]
    c[key] = c[key].copy()
    c[key][t] = value
    if t < 64:
        c["j"] = c["j"].copy()
        c["j"][64] = 1 << 50                      # a later violation too: the lowest triplet is the one reported
    g = Group(gpu_device, _three(gpu_device, c=c))
    assert g.call(65) == EINVAL
    msg = _lib.lib().rk_last_error()
    assert b"member 1" in msg and b"rule" in msg
    assert g.status_words().tolist() == [[0, -1], [rule, t], [0, -1]] and g.margins_intact()
    for a in g.members:
        K._untouched(a)
