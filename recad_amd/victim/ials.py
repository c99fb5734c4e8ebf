"""iALS victim on MI355X: weighted matrix factorisation for implicit feedback fitted by alternating least squares (Hu, Koren and
Volinsky 2008, "Collaborative Filtering for Implicit Feedback Datasets"): confidence c_ui = 1 + alpha q_ui on the stored entries
and 1 elsewhere, preference 1 / 0, and per row the normal equations (Y^T Y + lambda I + sum_e w_e y y^T) x_u = sum_e c_e y.

It is not in the reference.  include/recad_hip.h states the exact definition (the Gram matrix and A_u under rounding budgets, b_u
to the bit, an fp32 Cholesky solve inside LDS), csrc/ials.hip computes it, and tests/_ials_restate.py restates it in numpy.  ALS has
no sampler and no learning rate: given the initial item table (drawn from ``seed``) a fit is a deterministic function of the
ratings, and two fits give the same bits.  Unlike ``ease`` and ``itemknn`` it is an embedding model: it scores through
``scoring_tables()``, that is through rk_score_topk and the EvalSession replay, and it holds no I x I matrix.

``train_step`` runs one full sweep (users from items over the CSR, items from the new users over the transpose) and returns the
objective per (user, item) pair, evaluated in float64 on the device.  ``user_emb`` and ``item_emb`` are frozen parameters and
``sweeps_done`` a buffer, so ``.to()``, ``state_dict()`` and ``reset()`` behave as for the trained victims.

Conditioning: the solve is fp32, and the relative error of x_u is about 0.2 * kappa_2(A_u) * 2^-24, with
kappa ~ 1 + (|Y^T Y| + alpha sum_e q_e |y_e|^2) / lambda.  The defaults (alpha = 40 of Hu et al. section 4, lambda = 10) keep kappa
near 1e3 and the error near 2e-4; alpha = 40 with lambda = 0.5, or lambda = 0.01 with fewer rows than factors, reaches kappa 1e6
and an error of 1e-1, and can end in a refusal (a pivot that is not positive: rule 7).  That is inherent to fp32 ALS."""
import math

import torch
import torch.nn as nn

from .. import _lib
from .._ratings import DeviceRatings, checked_norms, transposed
from ..utils import VarDim
from .base import BaseVictim


def _f32(x):
    return torch.tensor(float(x), dtype=torch.float32).item()       # what the kernel receives


def _number(x):
    return not isinstance(x, bool) and isinstance(x, (int, float))


def check_config(factor_num, alpha, reg_lambda, init_std=0.01, seed=None):
    """The host-side refusals (ValueError), before any device call."""
    if isinstance(factor_num, bool) or not isinstance(factor_num, int) or not 1 <= factor_num <= _lib.RK_IALS_MAX_DIM:
        raise ValueError(f"iALS: factor_num = {factor_num!r}, expected an integer in 1..{_lib.RK_IALS_MAX_DIM}")
    if not (_number(alpha) and math.isfinite(_f32(alpha)) and _f32(alpha) >= 0):
        raise ValueError(f"iALS: alpha = {alpha!r}, expected a finite fp32 number >= 0")
    if not (_number(reg_lambda) and math.isfinite(_f32(reg_lambda)) and _f32(reg_lambda) > 0):
        raise ValueError(f"iALS: reg_lambda = {reg_lambda!r}, expected a finite fp32 number > 0")
    if not (_number(init_std) and math.isfinite(_f32(init_std)) and _f32(init_std) >= 0):
        raise ValueError(f"iALS: init_std = {init_std!r}, expected a finite fp32 number >= 0")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 63):
        raise ValueError(f"iALS: seed = {seed!r}, expected None or an integer in [0, 2^63)")


class IALS(BaseVictim):
    victim_name = "ials"

    def _build(self, factor_num, alpha, reg_lambda, init_std, seed, **config):
        self.dataset = config["dataset"]
        self.config = config
        info = self.dataset.info_describe()
        self.num_users, self.num_items = int(info["n_users"]), int(info["n_items"])
        self.dim, self.alpha, self.reg_lambda, self.init_std, self.seed = factor_num, alpha, reg_lambda, init_std, seed
        try:
            self._check()
            U, I, d = self.num_users, self.num_items, int(factor_num)
        except (ValueError, TypeError):
            U = I = d = 0                 # the refusal is raised by the first call that would use the tables
        if d and seed is None:
            self.seed = int(torch.randint(0, 2 ** 62, (1,)).item())     # from the global RNG, at .I()
        item = torch.zeros(I, d, dtype=torch.float32)
        if d:
            gen = torch.Generator().manual_seed(self.seed)
            item = torch.randn(I, d, generator=gen, dtype=torch.float32) * float(init_std)
        self.user_emb = nn.Parameter(torch.zeros(U, d, dtype=torch.float32), requires_grad=False)
        self.item_emb = nn.Parameter(item, requires_grad=False)
        self.register_buffer("user_bias", torch.zeros(U, dtype=torch.float32))
        self.register_buffer("item_bias", torch.zeros(I, dtype=torch.float32))
        self.register_buffer("sweeps_done", torch.zeros(1, dtype=torch.int64))
        self._csr = None                  # (device, CSR, transpose, the two row orders) of the dataset's rating matrix

    # ------------------------------------------------------------------ the ratings
    def _check(self):
        check_config(self.dim, self.alpha, self.reg_lambda, self.init_std, self.seed)
        if self.num_users < 1 or self.num_items < 1:
            raise ValueError(f"iALS: an empty catalogue ({self.num_users} users x {self.num_items} items)")

    def _device(self):
        dev = self.item_emb.device
        if dev.type != "cuda":
            raise _lib.HipCallError("iALS tables are on the CPU: call .to('cuda') first (no CPU fallback)")
        return dev

    def _ratings(self, dev):
        """The validated CSR, its transpose, and both sides' rows ordered longest first, cached per device."""
        if self._csr is None or self._csr[0] != dev:
            U, I = self.num_users, self.num_items
            rowptr, col, val = DeviceRatings(self.dataset, U, I, "iALS").on(dev)
            checked_norms("iALS", "rating matrix", U, I, rowptr, col, val)              # rules 1, 2, 3, 4
            colptr, crow, cval = transposed(U, I, rowptr, col, val)
            longest = lambda ptr: torch.argsort(ptr[1:] - ptr[:-1], descending=True, stable=True).to(torch.int32).contiguous()
            self._csr = (dev, (rowptr, col, val), (colptr, crow, cval), longest(rowptr), longest(colptr))
        return self._csr[1:]

    # ------------------------------------------------------------------ the fit
    def train_step(self, **config):
        """One sweep: X from Y over the CSR, Y from the new X over the transpose -> (J / (U * I),), J the objective of the new
        tables in float64.  A device refusal raises ValueError with the rule and the row and leaves the tables as they were."""
        self._check()
        dev = self._device()
        _lib.require_gpu()
        pbar = config.get("progress_bar", None)
        U, I, d = self.num_users, self.num_items, int(self.dim)
        alpha, lam = float(self.alpha), float(self.reg_lambda)
        csr, csc, order_u, order_i = self._ratings(dev)
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
        dp = (d + 15) // 16 * 16
        blocks = (max(U, I) + _lib.RK_IALS_GRAM_ROWS - 1) // _lib.RK_IALS_GRAM_ROWS
        work = torch.empty(blocks * dp * dp, dtype=torch.float32, device=dev)
        G = torch.empty(d * d, dtype=torch.float32, device=dev)
        X, Y = torch.empty_like(self.user_emb.data), torch.empty_like(self.item_emb.data)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        Y0 = self.item_emb.data
        _lib.check(L.rk_ials_gram(I, d, P(Y0), lam, P(G), P(work), work.numel(), s), "rk_ials_gram")
        _lib.check(L.rk_ials_half_sweep(U, I, d, P(G), P(csr[0]), P(csr[1]), P(csr[2]), alpha, P(Y0), P(order_u), P(X), P(status[0:2]), s),
                   "rk_ials_half_sweep")
        _lib.check(L.rk_ials_gram(U, d, P(X), lam, P(G), P(work), work.numel(), s), "rk_ials_gram")
        _lib.check(L.rk_ials_half_sweep(I, U, d, P(G), P(csc[0]), P(csc[1]), P(csc[2]), alpha, P(X), P(order_i), P(Y), P(status[2:4]), s),
                   "rk_ials_half_sweep")
        GY = torch.empty(d * d, dtype=torch.float64, device=dev)
        part = torch.empty(U, dtype=torch.float64, device=dev)
        J = torch.empty(1, dtype=torch.float64, device=dev)
        _lib.check(L.rk_ials_gram64(I, d, P(Y), P(GY), s), "rk_ials_gram64")
        _lib.check(L.rk_ials_objective(U, I, d, P(csr[0]), P(csr[1]), P(csr[2]), alpha, lam, P(X), P(Y), P(GY), P(part), P(J), s),
                   "rk_ials_objective")
        st = status.cpu().tolist()        # the one read of the status words: both half-sweeps
        for (rule, row), side in ((st[0:2], "user"), (st[2:4], "item")):
            if rule:
                raise ValueError(f"iALS: rule {rule} (a Cholesky pivot that is not a finite number > 0: the system is not positive "
                                 f"definite in fp32), first in {side} row {row}")
        self.user_emb.data.copy_(X)
        self.item_emb.data.copy_(Y)
        self.sweeps_done += 1
        loss = float(J.item()) / (float(U) * float(I))
        if pbar:
            pbar.set_description(f"loss: {loss:.6f}")
        return (loss,)

    # ------------------------------------------------------------------ scoring
    def _tables(self):
        self._check()
        self._device()
        return self.user_emb.data, self.item_emb.data, self.user_bias, self.item_bias

    def forward(self, users, items):
        ue, ie, ub, ib = self._tables()
        n = users.numel()
        out = torch.empty(n, device=ue.device, dtype=torch.float32)
        _lib.check(_lib.lib().rk_pair_scores(
            int(self.dim), _lib.ptr(ue), _lib.ptr(ie), _lib.ptr(ub), _lib.ptr(ib), 0.0, _lib.ptr(users.long().contiguous()),
            _lib.ptr(items.long().contiguous()), n, _lib.ptr(out), 0.0, 0, _lib.stream_ptr(ue.device)), "rk_pair_scores")
        return out

    scoring_tables_static = True   # views of the parameters, no launches: evaluate.EvalSession asks once and keeps them

    def scoring_tables(self):
        """Tables for the dot-product scoring path: zero biases, mean 0.0."""
        ue, ie, ub, ib = self._tables()
        return ue, ie, ub, ib, 0.0

    def scoring_tables_key(self):
        """Storage and shape of the four tables (evaluate.EvalSession compares it on every run())."""
        return (tuple((t.data_ptr(), tuple(t.shape)) for t in self._tables()),)

    def input_describe(self):
        return {
            "train_step": {},
            "forward": {"users": (torch.int64, (VarDim(comment="batch"))), "items": (torch.int64, (VarDim(comment="batch")))},
        }

    def output_describe(self):
        return {
            "train_step": {"loss": (float, [])},   # the objective J of the new tables, per (user, item) pair
            "forward": {"unnormalized_scores": (torch.float32, [VarDim(comment="batch")])},
        }
