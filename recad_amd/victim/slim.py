"""SLIM victim on MI355X: sparse linear item-item weights (Ning and Karypis 2011, "SLIM: Sparse Linear Methods for Top-N
Recommender Systems").  Each item's column of W is an elastic-net regression on the other items with non-negative weights and a
zero diagonal; score(u, .) = x_u W.

It is not in the reference, whose victims are all trained embedding models.  include/recad_hip.h states the exact definition
(the integer Gram matrix with l2_reg on its diagonal, cyclic coordinate descent in fp32 with every operation rounded on its own,
scores as EASE's fp32 chain in column order), csrc/slim.hip computes it one workgroup per column with the column's state in LDS,
and tests/_slim_restate.py restates it in numpy.  The fit has no sampler, no initialisation and no learning rate: two fits of
the same data give the same bits, to the last one.

"Training" is the fit: ``train_step`` builds W on first use and does nothing afterwards.  ``W`` is a frozen parameter and
``fitted`` a buffer, so ``.to()``, ``state_dict()`` and ``next(victim.parameters()).device`` behave as for the trained victims.
The Gram matrix is a temporary of the fit: a fit holds two I x I matrices.  W is oriented like EASE's B and scored by the same
entries.  The ratings themselves come from the dataset."""
import math

import torch
import torch.nn as nn

from .. import _lib
from ..utils import VarDim
from .base import BaseVictim


def _as_f32(x):
    return torch.tensor(float(x), dtype=torch.float32).item()       # what the kernel receives


def check_config(l1_reg, l2_reg, sweeps):
    """The host-side refusals (ValueError), before any device call."""
    ok = not isinstance(l1_reg, bool) and isinstance(l1_reg, (int, float))
    if ok:
        ok = math.isfinite(_as_f32(l1_reg)) and _as_f32(l1_reg) >= 0
    if not ok:
        raise ValueError(f"SLIM: l1_reg = {l1_reg!r}, expected a finite fp32 number >= 0")
    ok = not isinstance(l2_reg, bool) and isinstance(l2_reg, (int, float))
    if ok:
        ok = math.isfinite(_as_f32(l2_reg)) and _as_f32(l2_reg) > 0
    if not ok:
        raise ValueError(f"SLIM: l2_reg = {l2_reg!r}, expected a finite fp32 number > 0")
    if isinstance(sweeps, bool) or not isinstance(sweeps, int) or not 1 <= sweeps <= 2 ** 31 - 1:
        raise ValueError(f"SLIM: sweeps = {sweeps!r}, expected an integer >= 1")


class SLIM(BaseVictim):
    victim_name = "slim"

    def _build(self, l1_reg, l2_reg, sweeps, **config):
        self.dataset = config["dataset"]
        self.config = config
        info = self.dataset.info_describe()
        self.num_users, self.num_items = int(info["n_users"]), int(info["n_items"])
        self.l1_reg, self.l2_reg, self.sweeps = l1_reg, l2_reg, sweeps
        try:
            self._check()
            rows = self.num_items
        except (ValueError, TypeError):
            rows = 0                      # the refusal is raised by the first call that would use W
        self.W = nn.Parameter(torch.zeros(rows, rows, dtype=torch.float32), requires_grad=False)
        self.register_buffer("fitted", torch.zeros(1, dtype=torch.int32))
        self._csr = None                  # (device, rowptr, col, val) of the dataset's rating matrix
        self._info = None                 # int32 [I, 3] of the last fit this object ran

    # ------------------------------------------------------------------ the ratings
    def _check(self):
        check_config(self.l1_reg, self.l2_reg, self.sweeps)
        if not 1 <= self.num_items <= _lib.RK_SLIM_MAX_ITEMS:
            raise ValueError(f"SLIM: {self.num_items} items, a column's residual and weights live in one workgroup's LDS, which holds a "
                             f"catalogue of 1..{_lib.RK_SLIM_MAX_ITEMS} at most (the yelp-shaped catalogue is out of reach)")

    def _device(self):
        dev = self.W.device
        if dev.type != "cuda":
            raise _lib.HipCallError("SLIM weights are on the CPU: call .to('cuda') first (no CPU fallback)")
        return dev

    def _ratings(self, dev):
        from ..defense.pca_select_users import rating_csr

        if self._csr is None or self._csr[0] != dev:
            U, I, rowptr, col, val = rating_csr(self.dataset, dev)
            if (U, I) != (self.num_users, self.num_items):
                raise ValueError(f"SLIM: the dataset's rating matrix is {U} x {I}, its description says {self.num_users} x {self.num_items}")
            if col.numel() == 0:          # an empty matrix still needs addresses
                col, val = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.float32, device=dev)
            self._csr = (dev, rowptr, col, val)
        return self._csr[1:]

    # ------------------------------------------------------------------ the fit
    def fit(self):
        """Builds W from the dataset's rating matrix, whether or not it was built before.  A device refusal raises ValueError
        with the rule and the row or item, and leaves the model unfitted."""
        self._check()
        dev = self._device()
        _lib.require_gpu()
        U, I = self.num_users, self.num_items
        rowptr, col, val = self._ratings(dev)
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
        self.fitted.zero_()
        self._known_fit = False
        self._info = None
        nnz = int(col.numel())
        colptr = torch.empty(I + 1, dtype=torch.int32, device=dev)
        crow = torch.empty(nnz, dtype=torch.int32, device=dev)
        cval = torch.empty(nnz, dtype=torch.float32, device=dev)
        rnorm = torch.empty(U, dtype=torch.float32, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)

        def refused(rc, what):
            """(rule, index) of a device refusal, None when the call succeeded; any other failure raises HipCallError."""
            if rc == 0:
                return None
            rule, index = status.cpu().tolist()
            if not rule:
                _lib.check(rc, what)
            return rule, index

        bad = refused(L.rk_knn_norms(U, I, P(rowptr), P(col), P(val), P(rnorm), P(status), s), "rk_knn_norms")   # rules 1, 2, 3, 4
        if bad:
            raise ValueError(f"SLIM: the rating matrix breaks rule {bad[0]} ({_lib.RK_KNN_RULES.get(bad[0], '?')}), first in row {bad[1]}")
        _lib.check(L.rk_pca_transpose(U, I, P(rowptr), P(col), P(val), P(colptr), P(crow), P(cval), s), "rk_pca_transpose")
        G = torch.empty(I * I, dtype=torch.float32, device=dev)       # the fit's temporary: the second I x I matrix
        bad = refused(L.rk_ease_gram(U, I, P(rowptr), P(col), P(val), P(colptr), P(crow), P(cval), float(self.l2_reg), P(G), P(status), s),
                      "rk_ease_gram")
        if bad:
            raise ValueError(f"SLIM: the rating matrix breaks rule {bad[0]} (an item's squared norm of 2^24 or more), first in item {bad[1]}")
        info = torch.empty(I, 3, dtype=torch.int32, device=dev)
        bad = refused(L.rk_slim_fit(I, P(G), float(self.l1_reg), int(self.sweeps), P(self.W.data), P(info), None, P(status), s), "rk_slim_fit")
        if bad:
            raise ValueError(f"SLIM: rule {bad[0]} (a diagonal entry of the regularised Gram matrix is not a finite number > 0), at item {bad[1]}")
        self._info = info
        self.fitted.fill_(1)
        self._known_fit = True
        return self

    _known_fit = None                     # what `fitted` holds, once it has been read back; None: not known

    def _fitted_weights(self):
        self._check()
        dev = self._device()
        if self._known_fit is None:
            self._known_fit = bool(self.fitted.item())
        if not self._known_fit:
            self.fit()
        return dev, self.W.data

    def _load_from_state_dict(self, *args, **kwargs):
        self._known_fit = None            # `fitted` is about to be overwritten
        return super()._load_from_state_dict(*args, **kwargs)

    def train_step(self, **config):
        """Fits on first use and is a no-op afterwards (workflow.normal_train calls it rec_epoch times).  The fit has no loss
        to report: the value returned is 0.0."""
        self._fitted_weights()
        return (0.0,)

    def fit_info(self):
        """Per column (int32 [I] each, on the device): the last sweep that changed a coordinate (0: none did), the number of
        positive weights, and the number of coordinate steps that changed a weight.  The diagnostics belong to a fit this object
        ran: a model that is unfitted, or whose weights were loaded, is fitted first (the same bits)."""
        self._fitted_weights()
        if self._info is None:
            self.fit()
        last, support, steps = self._info.unbind(dim=1)
        return {"last_sweep": last, "support": support, "steps": steps}

    # ------------------------------------------------------------------ scoring
    def forward(self, users, items):
        dev, W = self._fitted_weights()
        rowptr, col, val = self._ratings(dev)
        users, items = users.long().contiguous(), items.long().contiguous()
        n = users.numel()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().rk_ease_pair_scores(
            self.num_items, self.num_users, _lib.ptr(W), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val),
            _lib.ptr(users) if n else None, _lib.ptr(items) if n else None, n, _lib.ptr(out) if n else None, _lib.stream_ptr(dev)),
            "rk_ease_pair_scores")
        return out

    def score_matrix(self, user_ids, out):
        """out[len(user_ids), n_items] <- the score of every item for each user (int32 ids on the device), seen items included;
        the batched evaluation then runs rk_topk_rows on it."""
        dev, W = self._fitted_weights()
        rowptr, col, val = self._ratings(dev)
        _lib.check(_lib.lib().rk_ease_scores(
            self.num_items, _lib.ptr(W), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), user_ids.numel(), _lib.ptr(user_ids), _lib.ptr(out),
            _lib.stream_ptr(dev)), "rk_ease_scores")

    def input_describe(self):
        return {
            "train_step": {},
            "forward": {"users": (torch.int64, (VarDim(comment="batch"))), "items": (torch.int64, (VarDim(comment="batch")))},
        }

    def output_describe(self):
        return {
            "train_step": {"loss": (float, [])},   # always 0.0: the fit reports no loss
            "forward": {"unnormalized_scores": (torch.float32, [VarDim(comment="batch")])},
        }
