"""AIA attacker on the device (recad/model/attacker/aia.py, registry recad/default.py:169-186).

Every train_step trains a fresh weighted-MF surrogate on the real rows and the fake ones for epoch_s epochs, then
differentiates the attack loss back through the last unroll_steps_s epochs' Adam steps to the fake profiles and takes one
Adam step on them.  csrc/aia.hip does the work: one launch per surrogate step over the batch's nonzeros of the data CSR
(the rating CSR plus filler_num slots per fake row), two per reverse step, two fused passes for the attack loss and its
gradient, one for the G step.  Nothing U x I, B x I or R x I is formed.

The generator is stored as attack_num x filler_num values at the template positions (columns ascending within a row).
This is exact: fake_parameter only matters under the template mask, and Adam leaves entries it never saw a gradient for at
exactly their initial value, which the mask multiplies by 0.

Random calls are the reference's, in its order, on the same generators: np.random.choice of the template users and one
np.random.shuffle per template at .I(); per train_step the WMF init (Q, then P, normal_(0, 0.1)) on torch's CPU default
generator and one np.random.shuffle of the row list per epoch, cumulative across epochs.  Seeding numpy and torch as a
reference run did reproduces its draws.

The reverse pass needs theta, m, v at every unrolled step.  They are all kept when (K + 1) slots fit history_bytes; otherwise
a checkpoint is kept every ceil(sqrt(K)) steps and each segment is re-run forward during the reverse pass.  The forward is
deterministic, so both give the same bits.

Deviation: a target every real user has rated raises ValueError (the reference returns NaN for it).
"""
import math

import numpy as np
import torch

from .. import _lib
from ..utils import VarDim
from ..victim.base import BaseVictim
from . import _common

_BETAS, _EPS = (0.9, 0.999), 1e-8      # torch.optim.Adam defaults (aia.py:66-68, 263-265)


def _dpad(d):
    return 16 if d <= 16 else (32 if d <= 32 else 64)


def draw_templates(ptr, idx, val, attack_num, filler_num):
    """build_network's draws (aia.py:54-63) on a rating CSR: np.random.choice over the users with at least filler_num
    positive ratings, then per template np.random.shuffle of its nonzero columns, the first filler_num kept.
    Returns (users [attack_num], columns [attack_num, filler_num] as drawn, in shuffle order)."""
    users, kept = _common.draw_templates(ptr, idx, val, attack_num, filler_num, need_filler_num=True)
    return users, np.asarray(kept, dtype=np.int64).reshape(attack_num, filler_num)


def target_pairs(ptr, idx, val, n_users, targets):
    """The (user, target) pairs of the attack loss: per target the real users with train_mat[u, t] == 0 (aia.py:92), grouped by
    target.  Returns (users, pair_ptr, target slot per pair, target id per pair, pidx [n_targets, n_users] = pair index or -1).
    A target every real user has rated is refused (the reference's loss is NaN there)."""
    rows = np.repeat(np.arange(n_users), np.diff(ptr))
    users, ptrs, slots, tg = [], [0], [], []
    pidx = np.full((len(targets), n_users), -1, dtype=np.int32)
    for s, t in enumerate(targets):
        rated = np.zeros(n_users, dtype=bool)
        rated[rows[(idx == t) & (val != 0)]] = True
        us = np.where(~rated)[0]
        if len(us) == 0:
            raise ValueError(f"AIA: every real user has rated target {t}; its attack loss is undefined (the reference returns NaN)")
        pidx[s, us] = len(users) + np.arange(len(us))
        users.extend(us.tolist())
        slots.extend([s] * len(us))
        tg.extend([t] * len(us))
        ptrs.append(len(users))
    return users, ptrs, slots, tg, pidx


class AIA(BaseVictim):
    """``model.from_config("attacker", "aia", **kw)`` keeps the configuration, ``.I(dataset=explicit)`` draws the templates,
    ``train_step(target_id_list=...)`` returns (G_loss,), ``generate_fake(target_id_list=...)`` returns an
    attack_num x n_items float32 array."""

    victim_name = "aia"
    scope = "attacker"

    def _build(self, attack_num, filler_num, lr_g, optim_g, surrogate_model, epoch_s, unroll_steps_s, hidden_dim_s, lr_s,
               weight_decay_s, batch_size_s, weight_pos_s, weight_neg_s, history_bytes, **config):
        self._refuse(config, surrogate_model, weight_neg_s, optim_g, hidden_dim_s, batch_size_s, unroll_steps_s, epoch_s, filler_num,
                     attack_num)
        ds, U, I, ptr, idx, val = _common.open_build(self, config)
        self.dataset = ds
        self.attack_num, self.filler_num = int(attack_num), int(filler_num)
        self.lr_g, self.lr_s, self.wd_s, self.w_pos = float(lr_g), float(lr_s), float(weight_decay_s), float(weight_pos_s)
        self.epoch_s, self.unroll, self.dim, self.batch = int(epoch_s), int(unroll_steps_s), int(hidden_dim_s), int(batch_size_s)
        self.history_bytes = int(history_bytes)
        self.n_users, self.n_items = U, I
        ptr, idx, val = np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(val, np.float32)
        self._host_csr = (ptr, idx, val)
        users, cols = draw_templates(ptr, idx, val, self.attack_num, self.filler_num)
        A, F = self.attack_num, self.filler_num
        order = np.argsort(cols, axis=1, kind="stable")
        scol = np.take_along_axis(cols, order, axis=1)
        tval = np.zeros((A, F), dtype=np.float32)
        for r, u in enumerate(users):
            b, e = ptr[u], ptr[u + 1]
            tval[r] = val[b:e][np.searchsorted(idx[b:e], scol[r])] if F else tval[r]
        self.template_users = users
        self.template_cols = scol                      # [A, F], ascending per row: the generator's positions
        self._surrogate_data(F * np.arange(1, A + 1, dtype=np.int64), scol.reshape(-1), A * F)
        self.gen = torch.as_tensor(tval.reshape(-1)).to(self.device)     # fake_parameter at the template positions
        self.gen_m = torch.zeros_like(self.gen)
        self.gen_v = torch.zeros_like(self.gen)
        self._g_t = 0
        self._project()
        self.last_entry = None
        self.last_xbar = None
        self.last_loss = None
        self.last_history = None

    def _refuse(self, config, surrogate_model, weight_neg_s, optim_g, hidden_dim_s, batch_size_s, unroll_steps_s, epoch_s, filler_num,
                attack_num):
        """The settings the surrogate attackers refuse, before a device is asked for; the message names the class being built."""
        name = type(self).__name__
        _common.need_dataset(self, config)
        if surrogate_model != "WMF":
            raise ValueError(f"{name}: surrogate_model {surrogate_model!r} is not supported (only 'WMF', as the reference)")
        if float(weight_neg_s) != 0.0:
            raise ValueError(f"{name}: weight_neg_s {weight_neg_s} is not supported (only 0: the loss stays on the positives)")
        if str(optim_g).lower() != "adam":
            raise ValueError(f"{name}: optim_g {optim_g!r} is not supported on the device (the reference's default 'adam' is)")
        if not 1 <= int(hidden_dim_s) <= 64:
            raise ValueError(f"{name}: hidden_dim_s {hidden_dim_s} must be in [1, 64]")
        if not 1 <= int(batch_size_s) <= _lib.RK_AIA_MAX_BATCH:
            raise ValueError(f"{name}: batch_size_s {batch_size_s} must be in [1, {_lib.RK_AIA_MAX_BATCH}]")
        if not 1 <= int(unroll_steps_s) <= int(epoch_s):
            raise ValueError(f"{name}: unroll_steps_s {unroll_steps_s} must be in [1, epoch_s = {epoch_s}]")
        if int(filler_num) < 0 or int(attack_num) <= 0:
            raise ValueError(f"{name}: attack_num must be positive and filler_num non-negative")

    def _surrogate_data(self, fake_ptr, fake_col, n_x):
        """The surrogate's data on the device: the rating CSR (self._host_csr), then the attack_num fake rows ending at
        nnz_real + fake_ptr with columns fake_col and n_x value slots (0 until the generator fills them).  Sets R, dpad, nnz_real,
        _rowptr, _col, _x, N, _desc and _pairs."""
        ptr, idx, val = self._host_csr
        dev, U, I = self.device, self.n_users, self.n_items
        self.R = R = U + self.attack_num
        self.dpad = _dpad(self.dim)
        rowptr = np.concatenate([ptr, ptr[-1] + fake_ptr])
        if rowptr[-1] >= 2 ** 31:
            raise ValueError(f"{type(self).__name__}: the surrogate's data has too many entries for int32 indices")
        self.nnz_real = int(ptr[-1])
        self._rowptr = torch.as_tensor(rowptr.astype(np.int32)).to(dev)
        self._col = torch.as_tensor(np.concatenate([idx, fake_col]).astype(np.int32)).to(dev)
        self._x = torch.as_tensor(np.concatenate([val, np.zeros(n_x, np.float32)])).to(dev)
        self.N = (R + I) * self.dpad
        d = _lib.AiaDesc()
        d.n_rows, d.n_real, d.n_items, d.dpad, d.batch, d.n_fake_nz = R, U, I, self.dpad, self.batch, len(fake_col)
        d.nnz_real = self.nnz_real
        d.rowptr, d.col, d.x = self._rowptr.data_ptr(), self._col.data_ptr(), self._x.data_ptr()
        d.lr, d.beta1, d.beta2, d.eps, d.wd, d.w_pos = self.lr_s, _BETAS[0], _BETAS[1], _EPS, self.wd_s, self.w_pos
        self._desc = d
        self._pairs = {}

    # ------------------------------------------------------------------ description (aia.py:72-86)
    def forward(self):
        pass

    def input_describe(self):
        return {"train_step": {"target_id_list": (list, VarDim())}}

    def output_describe(self):
        return {"train_step": {"g_losses": (float, [])}}

    # ------------------------------------------------------------------ plumbing
    def _s(self):
        return _lib.stream_ptr(self.device)

    def _project(self):
        n = self.gen.numel()
        if n:
            _lib.check(_lib.lib().rk_aia_project(n, _lib.ptr(self.gen), _lib.ptr(self._x[self.nnz_real:]), self._s()), "rk_aia_project")

    def generator_values(self):
        """fake_parameter at the template positions, [attack_num, filler_num] (columns: template_cols)."""
        return self.gen.cpu().numpy().reshape(self.attack_num, self.filler_num)

    def _targets(self, target_id_list):
        key = tuple(int(t) for t in target_id_list)
        if key in self._pairs:
            return self._pairs[key]
        if not key:
            raise ValueError("AIA: target_id_list is empty")
        U, I = self.n_users, self.n_items
        if min(key) < 0 or max(key) >= I:
            raise ValueError(f"AIA: target ids must lie in [0, {I})")
        users, ptrs, slots, tg, pidx = target_pairs(*self._host_csr, U, key)
        scale = np.asarray([1.0 / (11.0 * (ptrs[s + 1] - ptrs[s])) for s in range(len(key))], dtype=np.float32)
        dev = self.device
        i32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32)).to(dev)   # noqa: E731
        p = {"tgt": i32(key), "ptr": i32(ptrs), "user": i32(users), "ptgt": i32(tg), "slot": i32(slots), "pidx": i32(pidx.reshape(-1)),
             "scale": torch.as_tensor(scale).to(dev), "n": len(users), "key": key}
        self._pairs[key] = p
        return p

    def _perms(self, idx_list, n_epochs):
        """n_epochs in-place np.random.shuffle calls on idx_list (aia.py:444, 464) -> perms and inverses, [n_epochs, R] each."""
        perms = np.empty((n_epochs, self.R), dtype=np.int32)
        for e in range(n_epochs):
            np.random.shuffle(idx_list)
            perms[e] = idx_list
        inv = np.empty_like(perms)
        for e in range(n_epochs):
            inv[e, perms[e]] = np.arange(self.R, dtype=np.int32)
        return perms, inv

    def init_surrogate(self):
        """WeightedMF.__init__ (aia.py:229-236): Q [I, d] then P [R, d], normal_(0, 0.1) on torch's CPU default generator.
        Returns theta in the device layout (float32 [(R + I) * dpad], pad columns 0)."""
        Q = torch.zeros([self.n_items, self.dim]).normal_(mean=0, std=0.1)
        P = torch.zeros([self.R, self.dim]).normal_(mean=0, std=0.1)
        th = torch.zeros(self.R + self.n_items, self.dpad)
        th[: self.R, : self.dim] = P
        th[self.R:, : self.dim] = Q
        return th.reshape(-1)

    def state_to_numpy(self, slot):
        """(P [R, d], Q [I, d]) of a theta (or m, v) in the device layout."""
        a = slot.reshape(self.R + self.n_items, self.dpad)[:, : self.dim].cpu().numpy()
        return a[: self.R], a[self.R:]

    def _nsteps(self):
        return (self.R + self.batch - 1) // self.batch

    def _fwd(self, perm, inv, lo, hi, t_lo, slots, keep_all, parity0=0):
        _lib.check(_lib.lib().rk_aia_forward(_lib.C.byref(self._desc), _lib.ptr(perm), _lib.ptr(inv), lo, hi, t_lo, _lib.ptr(slots),
                                             int(keep_all), parity0, self._s()), "rk_aia_forward")

    def _pieces(self, a, b):
        """Global unrolled steps [a, b) split by epoch: (epoch, lo, hi)."""
        nb, out, g = self._nsteps(), [], a
        while g < b:
            e = g // nb
            h = min(b, (e + 1) * nb)
            out.append((e, g - e * nb, h - e * nb, g))
            g = h
        return out

    # ------------------------------------------------------------------ the surrogate (aia.py:421-489)
    def run_plain(self, theta0, perms, invs):
        """The detached epochs from theta0 (m = v = 0, step 0): returns (state [3N], adam steps taken)."""
        N, nb = self.N, self._nsteps()
        buf = torch.zeros(2, 3 * N, dtype=torch.float32, device=self.device)
        buf[0, :N] = theta0.to(self.device)
        par, t = 0, 0
        for e in range(perms.shape[0]):
            self._fwd(perms[e], invs[e], 0, nb, t + 1, buf, False, par)
            par = (par + nb) & 1
            t += nb
        return buf[par].clone(), t

    def unrolled(self, state, adam_t, perms, invs, target_id_list, history_bytes=None):
        """The unrolled epochs, the attack loss and the reverse pass from a given surrogate state: state [3N] = theta, m, v in the
        device layout after adam_t steps; perms / invs [n_unrolled_epochs, R] int32 device tensors.  Uses the current
        generator's projection for the fake rows.  Returns (G_loss device scalar, xbar [attack_num * filler_num] device,
        final theta [N])."""
        cap = self.history_bytes if history_bytes is None else int(history_bytes)
        N, dev, L, P = self.N, self.device, _lib.lib(), _lib.ptr
        K = perms.shape[0] * self._nsteps()
        slot_bytes = 3 * N * 4
        full = (K + 1) * slot_bytes <= cap
        S = K if full else max(1, math.ceil(math.sqrt(K)))
        segs = [(a, min(a + S, K)) for a in range(0, K, S)]
        self.last_history = {"full": full, "segment": S, "steps": K}
        if full:
            hist = torch.empty(K + 1, 3 * N, dtype=torch.float32, device=dev)
            hist[0] = state
            for e, lo, hi, g in self._pieces(0, K):
                self._fwd(perms[e], invs[e], lo, hi, adam_t + g + 1, hist[g], True)
            final = hist[K, :N]
        else:
            ck = torch.empty(len(segs), 3 * N, dtype=torch.float32, device=dev)
            pp = torch.empty(2, 3 * N, dtype=torch.float32, device=dev)
            pp[0] = state
            par = 0
            for c, (a, b) in enumerate(segs):
                ck[c] = pp[par]
                for e, lo, hi, g in self._pieces(a, b):
                    self._fwd(perms[e], invs[e], lo, hi, adam_t + g + 1, pp, False, par)
                    par = (par + hi - lo) & 1
            final = pp[par, :N]
            hist = torch.empty(S + 1, 3 * N, dtype=torch.float32, device=dev)
        pr = self._targets(target_id_list)
        work = torch.empty(3 * pr["n"], dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        adj = torch.empty(3 * N, dtype=torch.float32, device=dev)
        _lib.check(L.rk_aia_attack_loss(_lib.C.byref(self._desc), len(pr["key"]), P(pr["tgt"]), P(pr["ptr"]), pr["n"], P(pr["user"]),
                                        P(pr["ptgt"]), P(pr["slot"]), P(pr["pidx"]), P(pr["scale"]), P(final.contiguous()), P(work),
                                        P(loss), P(adj), self._s()), "rk_aia_attack_loss")
        gbar = torch.empty(N, dtype=torch.float32, device=dev)
        xbar = torch.zeros(max(1, self.gen.numel()), dtype=torch.float32, device=dev)
        for c in range(len(segs) - 1, -1, -1):
            a, b = segs[c]
            if not full:
                hist[0] = ck[c]
                for e, lo, hi, g in self._pieces(a, b):
                    self._fwd(perms[e], invs[e], lo, hi, adam_t + g + 1, hist[g - a], True)
            for e, lo, hi, g in reversed(self._pieces(a, b)):
                _lib.check(L.rk_aia_reverse(_lib.C.byref(self._desc), P(perms[e]), P(invs[e]), lo, hi, adam_t + g + 1,
                                            P(hist[g - a if not full else g]), P(adj), P(gbar), P(xbar), self._s()), "rk_aia_reverse")
        return loss, xbar[: self.gen.numel()], final.clone()

    # ------------------------------------------------------------------ aia.py:88-114
    def train_step(self, **config):
        """One G step: a fresh surrogate (epoch_s epochs, the last unroll_steps_s unrolled), the attack loss, its gradient at
        the fake profiles through the unrolled steps, one Adam step on the generator.  Returns (G_loss,)."""
        target_id_list = config["target_id_list"]
        self._targets(target_id_list)             # refuse bad targets before any draw
        self._project()
        theta0 = self.init_surrogate()
        idx_list = np.arange(self.R)
        E, K_e = self.epoch_s, self.unroll
        perms, invs = self._perms(idx_list, E)
        dp = torch.as_tensor(perms).to(self.device)
        di = torch.as_tensor(invs).to(self.device)
        state, t = self.run_plain(theta0, dp[: E - K_e], di[: E - K_e])
        self.last_entry = {"state": state, "adam_t": t, "perms": perms[E - K_e:].copy()}
        loss, xbar, _ = self.unrolled(state, t, dp[E - K_e:], di[E - K_e:], target_id_list)
        self.last_xbar = xbar
        self._g_t += 1
        _lib.check(_lib.lib().rk_aia_g_step(self.gen.numel(), _lib.ptr(self.gen), _lib.ptr(self.gen_m), _lib.ptr(self.gen_v),
                                            _lib.ptr(xbar) if xbar.numel() else None, self._g_t, self.lr_g, _BETAS[0], _BETAS[1],
                                            _EPS, self._s()), "rk_aia_g_step")
        self._project()
        g_loss = float(loss.cpu()[0])            # the step's one read-back
        self.last_loss = g_loss
        return (g_loss,)

    def entry_state(self):
        """The surrogate at entry to the unrolled epochs of the last train_step: dict of P, Q, mP, mQ, vP, vQ (numpy), adam_t,
        and the unrolled epochs' permutations."""
        st, N = self.last_entry["state"], self.N
        out = {"adam_t": self.last_entry["adam_t"], "perms": self.last_entry["perms"]}
        for k, name in enumerate(("", "m", "v")):
            out[name + "P"], out[name + "Q"] = self.state_to_numpy(st[k * N:(k + 1) * N])
        return out

    def last_hypergradient(self):
        """dG_loss / d fake at the template positions of the last train_step, [attack_num, filler_num]."""
        return self.last_xbar.cpu().numpy().reshape(self.attack_num, self.filler_num)

    # ------------------------------------------------------------------ aia.py:116-123
    def generate_fake(self, **kwargs):
        """project(fake_parameter * mask), each target set to 5 on its attack_num // len(targets) rows."""
        target_id_list = list(kwargs["target_id_list"])
        self._project()
        A, F = self.attack_num, self.filler_num
        x = self._x[self.nnz_real:].cpu().numpy().reshape(A, F)
        out = np.zeros((A, self.n_items), dtype=np.float32)
        if F:
            np.put_along_axis(out, self.template_cols, x, axis=1)
        rate = int(A / len(target_id_list))
        for i, t in enumerate(target_id_list):
            out[i * rate:(i + 1) * rate, int(t)] = 5
        return out
