"""GPU tests of the MF victim's two kernels (recad_amd/csrc/mf.hip) through rk_mf_train_epoch: the fused step per element against
the float64 restatement and its counted budgets (tests/_pointwise_restate.py: loss and the four gradient blocks, untouched rows
exactly +0.0, a dropped sample contributing exactly nothing), the dense Adam pass bit for bit against the oracle, the epoch loop's
step / mask numbering and its short last step, and the refusals.  Each test prints "RATIO <stage> <worst err / bound>" before it
asserts <= 1.  dim 1 / 63 / 64 / 65 / 130 puts the lane loop below, at and above one and two trips; 1025 and 1100 pairs take the
block loop's second trip."""
import ctypes as C

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


class Mf:
    def __init__(self, dev, c, state_seed=None, n_loss_steps=1):
        self.dev, self.c = dev, c
        self.tot = (c["n_users"] + c["n_items"]) * (c["dim"] + 1)
        self.bufs = []
        self.tab = [self._buf(c[k].size, c[k]) for k in ("ue", "ie", "ub", "ib")]
        rng = np.random.default_rng(0 if state_seed is None else state_seed)
        self.host_m = (0.1 * rng.standard_normal(self.tot)).astype(np.float32) if state_seed is not None else np.zeros(self.tot, np.float32)
        self.host_v = (1e-3 * rng.random(self.tot) + 1e-6).astype(np.float32) if state_seed is not None else np.zeros(self.tot, np.float32)
        self.m, self.v, self.g = self._buf(self.tot, self.host_m), self._buf(self.tot, self.host_v), self._buf(self.tot)
        self.loss = self._buf(n_loss_steps * _lib.RK_LOSS_PARTIALS)
        self.users, self.items, self.labels = (torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("users", "items", "labels"))

    def _buf(self, n, init=None):
        whole = torch.full((n + GUARD,), R.SENTINEL, device=self.dev)
        if init is not None:
            whole[:n].copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32).reshape(-1)))
        self.bufs.append((whole, n))
        return whole[:n]

    def guards_intact(self):
        return all(bool(np.all(w[n:].cpu().numpy().view(np.uint32) == SENT_BITS)) for w, n in self.bufs)

    def train(self, n=None, batch=None, adam_t0=0, apply=0, lo=0, dropout=0.0, lr=LR, **over):
        c = self.c
        n = len(c["users"]) - lo if n is None else n
        ptr = lambda t: C.c_void_p(t.data_ptr() + 8 * lo)
        a = dict(n_users=c["n_users"], n_items=c["n_items"], dim=c["dim"], ue=_lib.ptr(self.tab[0]), m=_lib.ptr(self.m), loss=_lib.ptr(self.loss), n=n,
                 batch=n if batch is None else batch)
        a.update(over)
        rc = _lib.lib().rk_mf_train_epoch(a["n_users"], a["n_items"], a["dim"], a["ue"], _lib.ptr(self.tab[1]), _lib.ptr(self.tab[2]), _lib.ptr(self.tab[3]),
                                          float(c["mean"]), a["m"], _lib.ptr(self.v), _lib.ptr(self.g), ptr(self.users), ptr(self.items), ptr(self.labels),
                                          a["n"], a["batch"], adam_t0, lr, B1, B2, EPS, a["loss"], apply, dropout, R.DROP_SEED, _lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc

    def params(self):
        return np.concatenate([t.cpu().numpy() for t in self.tab])

    def host_params(self):
        return np.concatenate([np.asarray(self.c[k], dtype=np.float32).reshape(-1) for k in ("ue", "ie", "ub", "ib")])


@pytest.mark.parametrize("p", R.MF_DROPS)
@pytest.mark.parametrize("nb", R.MF_NB)
@pytest.mark.parametrize("dim", R.MF_DIMS)
def test_mf_step(gpu_device, dim, nb, p):
    c = R.named_mf_case(dim, nb)
    assert float(c["mean"]) != 0
    m = Mf(gpu_device, c)
    assert m.train(adam_t0=5, dropout=p) == 0, _lib.lib().rk_last_error()
    assert m.guards_intact()
    loss = float(m.loss.cpu().numpy().astype(np.float64).sum())
    _report(R.check_mf_step(c, m.g.cpu().numpy(), loss, (p, R.DROP_SEED, 5) if p > 0 else None), prefix=f"d{dim}.nb{nb}.p{p}.")
    assert np.array_equal(R.bits(m.params()), R.bits(m.host_params())), "apply_update = 0 moved a parameter"


def _oracle_adam(p, g, m, v, t, lr=LR):
    p, m, v = (np.ascontiguousarray(a, dtype=np.float32).copy() for a in (p, m, v))
    orc.adam(p, np.ascontiguousarray(g, dtype=np.float32), m, v, t, lr, B1, B2, EPS)
    return p, m, v


@pytest.mark.parametrize("adam_t0", [0, 999])
def test_mf_adam_is_the_oracles_bits(gpu_device, adam_t0):
    d, nu, ni, nb = 65, 4099, 4001, 70
    edges = (nu * d, (nu + ni) * d, (nu + ni) * d + nu)
    assert all(e % 256 for e in edges) and edges[2] + ni > 2048 * 256, "a block must straddle every table boundary, and the grid stride twice"
    c = R.mf_case(d, nb, seed=9, n_users=nu, n_items=ni, hubs=False)
    assert len(np.unique(c["users"])) == nb and len(np.unique(c["items"])) == nb
    grads = []
    for _ in range(2):
        m = Mf(gpu_device, c, state_seed=4)
        assert m.train(adam_t0=adam_t0) == 0, _lib.lib().rk_last_error()
        grads.append(m.g.cpu().numpy())
    assert np.array_equal(R.bits(grads[0]), R.bits(grads[1])), "two apply_update = 0 runs differ"
    m = Mf(gpu_device, c, state_seed=4)
    assert m.train(adam_t0=adam_t0, apply=1) == 0, _lib.lib().rk_last_error()
    assert m.guards_intact()
    want = _oracle_adam(m.host_params(), grads[0], m.host_m, m.host_v, adam_t0 + 1)
    for name, got, ref in zip("pmv", (m.params(), m.m.cpu().numpy(), m.v.cpu().numpy()), want):
        assert np.array_equal(R.bits(got), R.bits(ref)), name
    assert not np.any(R.bits(m.g.cpu().numpy())), "the gradients are not +0.0 after the update"


def test_mf_epoch_numbers_masks_steps_and_the_short_tail(gpu_device):
    p, t0, n, B = 0.25, 5, 80, 32
    c = R.mf_case(63, n, seed=10, hubs=False)
    m = Mf(gpu_device, c, state_seed=6, n_loss_steps=3)
    assert m.train(n=n, batch=B, adam_t0=t0, apply=1, dropout=p, lr=0.0) == 0, _lib.lib().rk_last_error()
    assert m.guards_intact() and np.array_equal(R.bits(m.params()), R.bits(m.host_params())), "lr = 0 moved a parameter"
    epoch_loss = m.loss.cpu().numpy().reshape(3, 256)
    want_m, want_v = m.host_m, m.host_v
    for s, (lo, hi) in enumerate(((0, 32), (32, 64), (64, 80))):
        one = Mf(gpu_device, c)
        assert one.train(n=hi - lo, batch=B, adam_t0=t0 + s, lo=lo, dropout=p) == 0, _lib.lib().rk_last_error()
        row, g = one.loss.cpu().numpy(), one.g.cpu().numpy()
        _report(R.check_mf_step(R.sub_case(c, lo, hi), g, float(row.astype(np.float64).sum()), (p, R.DROP_SEED, t0 + s)), prefix=f"epoch.step{s}.")
        assert np.array_equal(R.bits(epoch_loss[s]), R.bits(row)), f"loss row {s} of the epoch differs from the step on its own"
        _, want_m, want_v = _oracle_adam(m.host_params(), g, want_m, want_v, t0 + s + 1, lr=0.0)
    assert np.array_equal(R.bits(m.m.cpu().numpy()), R.bits(want_m)) and np.array_equal(R.bits(m.v.cpu().numpy()), R.bits(want_v))
    assert not np.any(R.bits(m.g.cpu().numpy()))


def test_mf_refusals_launch_nothing(gpu_device):
    c = R.mf_case(7, 20, seed=11)
    for what, kw in (("dim = 0", dict(dim=0)), ("n_users = 0", dict(n_users=0)), ("n = 0", dict(n=0)), ("batch = 0", dict(batch=0)),
                     ("dropout = 1", dict(dropout=1.0)), ("dropout < 0", dict(dropout=-0.1)), ("no tables", dict(ue=None)), ("no moments", dict(m=None)),
                     ("no loss partials", dict(loss=None))):
        m = Mf(gpu_device, c)
        assert m.train(**kw) == EINVAL and _lib.lib().rk_last_error(), what
        assert m.guards_intact() and all(bool(np.all(t.cpu().numpy().view(np.uint32) == SENT_BITS)) for t in (m.g, m.loss)), what
        assert np.array_equal(R.bits(m.params()), R.bits(m.host_params())), what
    m = Mf(gpu_device, c)
    assert m.train() == 0
