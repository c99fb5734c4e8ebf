"""PGA attacker on the device: projected gradient ascent on the fake profiles through a factorisation fitted by alternating
least squares (Li, Wang, Singh and Vorobeychik, "Data Poisoning Attacks on Factorization-Based Collaborative Filtering", NIPS
2016).  It is not in the reference.  include/recad_hip.h states the exact definition, csrc/pga.hip computes it and
tests/_pga_restate.py restates it in numpy.

The state is R in [0, 1]^{attack_num x n_items}, the inclusion strengths of the fake users, with the target columns pinned to 1.
The binarised profile of a row is the targets and the filler_num non-target items of largest strength (ties to the lower id),
every entry rated fake_rating.  R starts at 1 on the items of ``_common.draw_templates(..., need_filler_num=True)`` -- AIA's draws
from the same generators, so seeding numpy makes a run repeatable -- and 0 elsewhere.

Every ``train_step`` fits an ordinary iALS surrogate (rk_ials_gram, rk_ials_half_sweep; its own factor_num_s, alpha_s,
reg_lambda_s, seed_s) on the real ratings with the binarised fake rows appended: init_sweeps_s sweeps from the seeded item table
the first time, sweeps_s sweeps warm-started from the last tables afterwards.  The adversarial loss (the masked softmax
cross-entropy of the targets over the real users who have not rated them) is taken on the last sweep's tables, and its
hypergradient with respect to R is closed-form: two batches of the per-row solves the sweep itself runs (rk_ials_solve_rhs), one
d x d product, one sparse adjoint per fake row and one A x I pass.  Like ``aia``'s ``unroll_steps_s = 1`` it differentiates ONE
sweep (the item table the users were solved from is held constant), not the converged fixed point.  Then
R <- clip(R - lr * grad / max|grad|, 0, 1), the targets go back to 1 and the profiles are selected again.

The class only sequences the entries: no formula is restated here.  The surrogate sees every target in every fake row;
``generate_fake`` writes fake_rating at the selected fillers and 5 at each target on its attack_num // len(targets) rows, as the
other attackers do.

Refusals (ValueError, before a device is asked for): settings out of range, ratings that are not integers in 1..127, no user
with filler_num positive ratings, and per call: an empty, repeated or out-of-range target list, more than RK_PGA_MAX_TARGETS
targets, filler_num above the items that are no targets, a target every real user has rated."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from ..utils import VarDim, get_logger
from ..victim.base import BaseVictim
from . import _common

INIT_STD = 0.01            # the surrogate's seeded item table, as the ials victim's default


def _f32(x):
    return float(np.float32(x))


def _number(x):
    return not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating))


def _integer(x):
    return not isinstance(x, bool) and isinstance(x, (int, np.integer))


def check_config(attack_num, filler_num, fake_rating, lr, factor_num_s, alpha_s, reg_lambda_s, init_sweeps_s, sweeps_s, seed_s):
    """The host-side refusals of the settings (ValueError), before any device call."""
    if not _integer(attack_num) or attack_num < 1:
        raise ValueError(f"PGA: attack_num = {attack_num!r}, expected a positive integer")
    if not _integer(filler_num) or filler_num < 0:
        raise ValueError(f"PGA: filler_num = {filler_num!r}, expected a non-negative integer")
    if not (_number(fake_rating) and float(fake_rating) == int(fake_rating) and 1 <= int(fake_rating) <= 127):
        raise ValueError(f"PGA: fake_rating = {fake_rating!r}, expected an integer value in 1..127 (the rating CSR's rule)")
    if not (_number(lr) and math.isfinite(_f32(lr)) and _f32(lr) > 0):
        raise ValueError(f"PGA: lr = {lr!r}, expected a finite fp32 number > 0")
    if not _integer(factor_num_s) or not 1 <= factor_num_s <= _lib.RK_IALS_MAX_DIM:
        raise ValueError(f"PGA: factor_num_s = {factor_num_s!r}, expected an integer in 1..{_lib.RK_IALS_MAX_DIM}")
    if not (_number(alpha_s) and math.isfinite(_f32(alpha_s)) and _f32(alpha_s) >= 0):
        raise ValueError(f"PGA: alpha_s = {alpha_s!r}, expected a finite fp32 number >= 0")
    if not (_number(reg_lambda_s) and math.isfinite(_f32(reg_lambda_s)) and _f32(reg_lambda_s) > 0):
        raise ValueError(f"PGA: reg_lambda_s = {reg_lambda_s!r}, expected a finite fp32 number > 0")
    for name, v in (("init_sweeps_s", init_sweeps_s), ("sweeps_s", sweeps_s)):
        if not _integer(v) or v < 1:
            raise ValueError(f"PGA: {name} = {v!r}, expected a positive integer (the hypergradient needs a sweep to go through)")
    if seed_s is not None and (not _integer(seed_s) or not 0 <= seed_s < 2 ** 63):
        raise ValueError(f"PGA: seed_s = {seed_s!r}, expected None or an integer in [0, 2^63)")


def check_data(n_users, n_items, ptr, idx, val, attack_num, filler_num):
    """The refusals that need the ratings (ValueError), still before any device call."""
    if n_users < 1 or n_items < 2:
        raise ValueError(f"PGA: {n_users} users x {n_items} items; at least one user and two items are needed")
    if n_users + attack_num >= 2 ** 31 or len(idx) + attack_num * n_items >= 2 ** 31:
        raise ValueError("PGA: the surrogate's data has too many rows or entries for int32 indices")
    if filler_num > n_items - 1:
        raise ValueError(f"PGA: filler_num = {filler_num} leaves no room for a target among {n_items} items")
    val = np.asarray(val)
    if len(val) and not (np.all(val == np.floor(val)) and val.min() >= 1 and val.max() <= 127):
        raise ValueError("PGA: the ratings must be integers in 1..127 (the rule of the iALS entries)")
    cnt = np.bincount(np.repeat(np.arange(n_users), np.diff(ptr))[val > 0], minlength=n_users)
    if not np.any(cnt >= filler_num):
        raise ValueError(f"PGA: no user has {filler_num} positive ratings to draw a template from")


def check_targets(n_users, n_items, ptr, idx, filler_num, target_id_list):
    """The refusals of one target list (ValueError) -> (key, eligible [n_targets, n_users] bool).  A target every real user has
    rated has an empty E_t and no loss."""
    key = tuple(int(t) for t in target_id_list)
    if not key:
        raise ValueError("PGA: target_id_list is empty")
    if len(key) > _lib.RK_PGA_MAX_TARGETS:
        raise ValueError(f"PGA: {len(key)} targets, at most {_lib.RK_PGA_MAX_TARGETS}")
    if len(set(key)) != len(key):
        raise ValueError(f"PGA: target_id_list {list(key)} repeats an id")
    if min(key) < 0 or max(key) >= n_items:
        raise ValueError(f"PGA: target ids must lie in [0, {n_items})")
    if filler_num > n_items - len(key):
        raise ValueError(f"PGA: filler_num = {filler_num} exceeds the {n_items - len(key)} items that are no targets")
    rows = np.repeat(np.arange(n_users), np.diff(ptr))
    elig = np.ones((len(key), n_users), dtype=bool)
    for s, t in enumerate(key):
        elig[s, rows[np.asarray(idx) == t]] = False
        if not elig[s].any():
            raise ValueError(f"PGA: every real user has rated target {t}; its attack loss is undefined")
    return key, elig


class PGA(BaseVictim):
    """``model.from_config("attacker", "pga", **kw)`` keeps the configuration, ``.I(dataset=explicit)`` draws the templates,
    ``train_step(target_id_list=...)`` returns (adv_loss,), ``generate_fake(target_id_list=...)`` returns an
    attack_num x n_items float32 array."""

    victim_name = "pga"
    scope = "attacker"

    def _build(self, attack_num, filler_num, fake_rating, lr, factor_num_s, alpha_s, reg_lambda_s, init_sweeps_s, sweeps_s, seed_s,
               **config):
        ds = _common.need_dataset(self, config)
        check_config(attack_num, filler_num, fake_rating, lr, factor_num_s, alpha_s, reg_lambda_s, init_sweeps_s, sweeps_s, seed_s)
        U, I, ptr, idx, val = _common.train_csr(ds)
        ptr, idx, val = np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(val, np.float32)
        check_data(U, I, ptr, idx, val, attack_num, filler_num)
        _lib.require_gpu()
        self.logger = get_logger(type(self).__module__, level=config.get("logging_level", 20))
        self.device = dev = torch.device(config.get("device", "cuda"))
        self.dataset = ds
        self.attack_num, self.filler_num, self.fake_rating = int(attack_num), int(filler_num), float(int(fake_rating))
        self.lr, self.dim, self.alpha, self.reg_lambda = float(lr), int(factor_num_s), float(alpha_s), float(reg_lambda_s)
        self.init_sweeps, self.sweeps = int(init_sweeps_s), int(sweeps_s)
        self.n_users, self.n_items = U, I
        self.user_block = 2048                          # users whose score rows are held at once
        self._host_csr = (ptr, idx, val)
        users, kept = _common.draw_templates(ptr, idx, val, self.attack_num, self.filler_num, need_filler_num=True)
        self.template_users = users
        R0 = np.zeros((self.attack_num, I), dtype=np.float32)
        for r, cols in enumerate(kept):
            R0[r, cols] = 1.0
        self.seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed_s is None else int(seed_s)
        gen = torch.Generator().manual_seed(self.seed)
        self._Y = (torch.randn(I, self.dim, generator=gen, dtype=torch.float32) * INIT_STD).to(dev)
        self._R = torch.as_tensor(R0).to(dev)
        self.nnz_real = int(ptr[-1])
        self._rowptr = torch.as_tensor(ptr.astype(np.int32)).to(dev)
        self._col = torch.as_tensor(idx.astype(np.int32)).to(dev)
        self._val = torch.as_tensor(val).to(dev)
        self.wbar = float(np.float32(self.alpha) * np.float32(self.fake_rating))
        self._targets_cache = {}
        self._profile = None                            # the binarised rows and the surrogate's data, for one target list
        self._fitted = False
        self._grad = self._tables = None
        self.last_loss = None

    # ------------------------------------------------------------------ description
    def forward(self):
        pass

    def input_describe(self):
        return {"train_step": {"target_id_list": (list, VarDim())}}

    def output_describe(self):
        return {"train_step": {"adv_loss": (float, [])}}

    # ------------------------------------------------------------------ plumbing
    def _s(self):
        return _lib.stream_ptr(self.device)

    def _gemm(self, M, N, K, a, a_rs, a_cs, b, b_rs, b_cs, c, ldc):
        """C[m, n] = sum_k A(m, k) B(n, k) through the library's fp32 MFMA dispatcher; a, b, c are device addresses."""
        g = _lib.GemmDesc()
        g.M, g.N, g.K, g.policy = M, N, K, _lib.RK_GEMM_POLICY_LAUNCH
        g.A, g.a_rs, g.a_cs = a, a_rs, a_cs
        g.B, g.b_rs, g.b_cs = b, b_rs, b_cs
        g.C, g.ldc = c, ldc
        _lib.check(_lib.lib().rk_gemm_f32(C.byref(g), None, None, self._s()), "rk_gemm_f32")

    def _targets(self, target_id_list):
        key = tuple(int(t) for t in target_id_list)
        if key not in self._targets_cache:
            ptr, idx, _ = self._host_csr
            key, elig = check_targets(self.n_users, self.n_items, ptr, idx, self.filler_num, target_id_list)
            dev = self.device
            self._targets_cache[key] = {"key": key, "tgt": torch.as_tensor(np.asarray(key, dtype=np.int32)).to(dev),
                                        "elig": torch.as_tensor(elig.astype(np.int32)).to(dev),
                                        "inv": [1.0 / float(e.sum()) for e in elig]}
        return self._targets_cache[key]

    def _open_profile(self, pr):
        """The surrogate's data for one target list: the rating CSR with attack_num rows of n_targets + filler_num entries
        appended (their columns are what rk_pga_step writes), and room for its transpose."""
        A, U, I, dev = self.attack_num, self.n_users, self.n_items, self.device
        ln = len(pr["key"]) + self.filler_num
        nnz = self.nnz_real + A * ln
        fptr = torch.arange(A + 1, dtype=torch.int64) * ln
        p = {"key": pr["key"], "len": ln, "nnz": nnz,
             "rowptr": torch.cat([self._rowptr.cpu().long(), self.nnz_real + fptr[1:]]).to(torch.int32).to(dev),
             "col": torch.cat([self._col, torch.zeros(A * ln, dtype=torch.int32, device=dev)]),
             "val": torch.cat([self._val, torch.full((A * ln,), self.fake_rating, dtype=torch.float32, device=dev)]),
             "fptr": fptr.to(torch.int32).to(dev),
             "colptr": torch.empty(I + 1, dtype=torch.int32, device=dev),
             "crow": torch.empty(nnz, dtype=torch.int32, device=dev), "cval": torch.empty(nnz, dtype=torch.float32, device=dev)}
        p["fcol"], p["fval"] = p["col"][self.nnz_real:], p["val"][self.nnz_real:]
        self._profile = p
        return p

    def _select(self, pr, update):
        """rk_pga_step (with the update when asked) and the transpose of the new data."""
        p = self._profile if self._profile is not None and self._profile["key"] == pr["key"] else self._open_profile(pr)
        L, P = _lib.lib(), _lib.ptr
        grad, gmax = (self._grad, self._gmax) if update else (None, None)
        _lib.check(L.rk_pga_step(self.attack_num, self.n_items, P(self._R), P(grad), P(gmax), self.lr, len(pr["key"]), P(pr["tgt"]),
                                 self.filler_num, P(p["fcol"]), self._s()), "rk_pga_step")
        _lib.check(L.rk_pca_transpose(self.n_users + self.attack_num, self.n_items, P(p["rowptr"]), P(p["col"]), P(p["val"]),
                                      P(p["colptr"]), P(p["crow"]), P(p["cval"]), self._s()), "rk_pca_transpose")
        return p

    def _fit(self, p, n_sweeps):
        """n_sweeps sweeps from self._Y; keeps Yo, X, Yp and the two Gram matrices of the last one."""
        U, A, I, d, dev = self.n_users, self.attack_num, self.n_items, self.dim, self.device
        L, P, s = _lib.lib(), _lib.ptr, self._s()
        n_rows = U + A
        dp = (d + 15) // 16 * 16
        blocks = (max(n_rows, I) + _lib.RK_IALS_GRAM_ROWS - 1) // _lib.RK_IALS_GRAM_ROWS
        work = torch.empty(blocks * dp * dp, dtype=torch.float32, device=dev)
        Go = torch.empty(d * d, dtype=torch.float32, device=dev)
        Gx = torch.empty(d * d, dtype=torch.float32, device=dev)
        status = torch.zeros(n_sweeps, 4, dtype=torch.int32, device=dev)
        Y = self._Y
        for k in range(n_sweeps):
            X = torch.empty(n_rows, d, dtype=torch.float32, device=dev)
            Yn = torch.empty(I, d, dtype=torch.float32, device=dev)
            _lib.check(L.rk_ials_gram(I, d, P(Y), self.reg_lambda, P(Go), P(work), work.numel(), s), "rk_ials_gram")
            _lib.check(L.rk_ials_half_sweep(n_rows, I, d, P(Go), P(p["rowptr"]), P(p["col"]), P(p["val"]), self.alpha, P(Y), None, P(X),
                                            P(status[k, 0:2]), s), "rk_ials_half_sweep")
            _lib.check(L.rk_ials_gram(n_rows, d, P(X), self.reg_lambda, P(Gx), P(work), work.numel(), s), "rk_ials_gram")
            _lib.check(L.rk_ials_half_sweep(I, n_rows, d, P(Gx), P(p["colptr"]), P(p["crow"]), P(p["cval"]), self.alpha, P(X), None,
                                            P(Yn), P(status[k, 2:4]), s), "rk_ials_half_sweep")
            Yo, Y = Y, Yn
        self._tables = {"Yo": Yo, "X": X, "Yp": Y, "Go": Go, "Gx": Gx}
        self._Y = Y
        return status

    def _loss(self, p, pr, tables):
        """The loss (a device double) and g [I, d] from the tables: per target and block of users the scores, rk_pga_loss, and
        the block's D^T X; then the partial products in order.  The real rows lead the surrogate's CSR, so it serves as theirs."""
        U, I, d, dev = self.n_users, self.n_items, self.dim, self.device
        L, P, s = _lib.lib(), _lib.ptr, self._s()
        X, Yp = tables["X"], tables["Yp"]
        B = min(int(self.user_block), U)
        blocks = [(u0, min(B, U - u0)) for u0 in range(0, U, B)]
        n_t = len(pr["key"])
        S = torch.empty(B * I, dtype=torch.float32, device=dev)
        parts = torch.empty(n_t * len(blocks), I * d, dtype=torch.float32, device=dev)
        terms = torch.empty(n_t * U, dtype=torch.float64, device=dev)
        k = 0
        for ti, t in enumerate(pr["key"]):
            for u0, nb in blocks:
                xb = X.data_ptr() + 4 * u0 * d
                self._gemm(nb, I, d, xb, d, 1, Yp.data_ptr(), d, 1, S.data_ptr(), I)
                _lib.check(L.rk_pga_loss(nb, I, P(S), P(p["rowptr"]), P(p["col"]), u0, t, P(pr["elig"][ti]), pr["inv"][ti],
                                         C.c_void_p(terms.data_ptr() + 8 * (ti * U + u0)), s), "rk_pga_loss")
                self._gemm(I, d, nb, S.data_ptr(), 1, I, xb, 1, d, parts[k].data_ptr(), d)
                k += 1
        g = torch.empty(I, d, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float64, device=dev)
        _lib.check(L.rk_pga_add_blocks(I * d, k, P(parts), P(g), s), "rk_pga_add_blocks")
        _lib.check(L.rk_pga_loss_sum(n_t * U, P(terms), P(loss), s), "rk_pga_loss_sum")
        return loss, g

    def _hypergradient(self, p, tables, g):
        """Z, M, H, V and the A x I gradient with its largest magnitude -> the status words of the two solves."""
        U, A, I, d, dev = self.n_users, self.attack_num, self.n_items, self.dim, self.device
        L, P, s = _lib.lib(), _lib.ptr, self._s()
        X, Yo, Yp = tables["X"], tables["Yo"], tables["Yp"]
        Xf = X[U:]
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)   # noqa: E731
        Z, M, H, V = new(I, d), new(d, d), new(A, d), new(A, d)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        _lib.check(L.rk_ials_solve_rhs(I, U + A, d, P(tables["Gx"]), P(p["colptr"]), P(p["crow"]), P(p["cval"]), self.alpha, P(X), P(g),
                                       None, P(Z), P(status[0:2]), s), "rk_ials_solve_rhs")
        self._gemm(d, d, I, Z.data_ptr(), 1, d, Yp.data_ptr(), 1, d, M.data_ptr(), d)
        _lib.check(L.rk_pga_user_adjoint(A, I, d, P(Z), P(Yp), P(Xf), P(M), P(p["fptr"]), P(p["fcol"]), self.wbar, P(H), s),
                   "rk_pga_user_adjoint")
        _lib.check(L.rk_ials_solve_rhs(A, I, d, P(tables["Go"]), P(p["fptr"]), P(p["fcol"]), P(p["fval"]), self.alpha, P(Yo), P(H), None,
                                       P(V), P(status[2:4]), s), "rk_ials_solve_rhs")
        if self._grad is None:
            self._grad, self._gmax = new(A, I), torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(L.rk_pga_grad(A, I, d, P(Xf), P(V), P(Z), P(Yp), P(Yo), self.wbar, P(self._grad), P(self._gmax), s), "rk_pga_grad")
        self._stages = {"g": g, "Z": Z, "M": M, "H": H, "V": V}
        return status

    # ------------------------------------------------------------------ the attacker's contract
    def train_step(self, **config):
        """One projected gradient step: the surrogate's sweeps on the current profiles, the adversarial loss, its hypergradient
        through the last sweep, the update of R and the new profiles.  Returns (adv_loss,), the loss BEFORE the update."""
        pr = self._targets(config["target_id_list"])           # refuses bad targets before anything is launched
        p = self._profile
        if p is None or p["key"] != pr["key"]:
            p = self._select(pr, update=False)
        st_fit = self._fit(p, self.sweeps if self._fitted else self.init_sweeps)
        self._fitted = True
        loss, g = self._loss(p, pr, self._tables)
        st_hyp = self._hypergradient(p, self._tables, g)
        self._select(pr, update=True)
        words = torch.cat([st_fit.reshape(-1), st_hyp]).cpu().tolist()      # the step's reads: the status words, then the loss
        for k in range(0, len(words), 2):
            if words[k]:
                raise ValueError(f"PGA: rule {words[k]} (a Cholesky pivot that is not a finite number > 0: the surrogate's system is "
                                 f"not positive definite in fp32), first in row {words[k + 1]} of solve {k // 2}")
        self.last_loss = float(loss.cpu()[0])
        if not math.isfinite(self.last_loss):
            raise ValueError(f"PGA: the adversarial loss is {self.last_loss}; the surrogate's tables are not finite")
        pbar = config.get("progress_bar", None)
        if pbar:
            pbar.set_description(f"adv_loss: {self.last_loss:.6f}")
        return (self.last_loss,)

    def generate_fake(self, **kwargs):
        """fake_rating at the selected fillers, each target set to 5 on its attack_num // len(targets) rows."""
        target_id_list = list(kwargs["target_id_list"])
        pr = self._targets(target_id_list)
        if self._profile is None or self._profile["key"] != pr["key"]:
            self._select(pr, update=False)
        A = self.attack_num
        out = np.zeros((A, self.n_items), dtype=np.float32)
        np.put_along_axis(out, self.profiles().astype(np.int64), np.float32(self.fake_rating), axis=1)
        out[:, list(pr["key"])] = 0
        rate = int(A / len(target_id_list))
        for i, t in enumerate(target_id_list):
            out[i * rate:(i + 1) * rate, int(t)] = 5
        return out

    # ------------------------------------------------------------------ what the tests and the curious read
    def last_gradient(self):
        """dL / dR of the last train_step, [attack_num, n_items]."""
        return self._grad.cpu().numpy()

    def strengths(self):
        """R, [attack_num, n_items]."""
        return self._R.cpu().numpy()

    def profiles(self):
        """The binarised rows: [attack_num, n_targets + filler_num] column ids, ascending per row."""
        return self._profile["fcol"].cpu().numpy().reshape(self.attack_num, self._profile["len"])

    def surrogate_tables(self):
        """The last sweep's tables as numpy: Yo [I, d], X [U + A, d] (the fake rows last), Yp [I, d]."""
        return {k: self._tables[k].cpu().numpy() for k in ("Yo", "X", "Yp")}

    def last_stages(self):
        """g, Z, M, H, V of the last train_step as numpy."""
        return {k: v.cpu().numpy() for k, v in self._stages.items()}
