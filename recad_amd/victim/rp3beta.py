"""RP3beta victim on MI355X: the random-walk item-item recommender (P3alpha: Cooper, Lee, Radzik and Siantos 2014; RP3beta:
Christoffel, Paudel, Newell and Bernstein 2015; Paudel et al. 2017), the one common model whose scores penalise popularity
(``beta`` > 0), which is what the bandwagon and popular-item attack profiles lean on.  ``beta`` = 0 is P3alpha.

It is not in the reference, whose victims are all trained embedding models.  include/recad_hip.h states the exact definition
(transition probabilities as 40-bit fixed-point integers, 64-bit integer dots, the weight formed in double and rounded once to
fp32, neighbours by (w descending, id ascending), the fp32 score summed in ascending item order), csrc/rp3beta.hip computes it
without an I x I matrix, and tests/_rp3_restate.py restates it in numpy, bit for bit.

Like ``ItemKNN`` it has no sampler, no initialisation and no epochs: ``train_step`` builds the neighbour tables on first use and
does nothing afterwards.  The tables are module state (``nbr_w`` a frozen parameter, ``nbr_id`` and ``fitted`` buffers)."""
import math

import torch
import torch.nn as nn

from .. import _lib
from ..utils import VarDim
from .base import BaseVictim


def _exponent_ok(x):
    return not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x) and 0.0 <= x <= 4.0


def check_config(alpha, beta, k, band, n_users=None):
    """The host-side refusals (ValueError), before any device call."""
    if not _exponent_ok(alpha):
        raise ValueError(f"RP3beta: alpha = {alpha!r}, expected a finite number in [0, 4]")
    if not _exponent_ok(beta):
        raise ValueError(f"RP3beta: beta = {beta!r}, expected a finite number in [0, 4]")
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= _lib.RK_KNN_MAX_K:
        raise ValueError(f"RP3beta: k = {k!r} outside 1..{_lib.RK_KNN_MAX_K}")
    if band is not None and (isinstance(band, bool) or int(band) != band or band % 64 or not 64 <= band <= _lib.RK_RP3_MAX_BAND):
        raise ValueError(f"RP3beta: band = {band!r}, expected None or a multiple of 64 in 64..{_lib.RK_RP3_MAX_BAND}")
    if n_users is not None and n_users >= _lib.RK_RP3_MAX_USERS:
        raise ValueError(f"RP3beta: {n_users} users, fewer than {_lib.RK_RP3_MAX_USERS} keep every 64-bit dot exact")


class RP3beta(BaseVictim):
    victim_name = "rp3beta"

    def _build(self, alpha, beta, k, band, **config):
        self.dataset = config["dataset"]
        self.config = config
        info = self.dataset.info_describe()
        self.num_users, self.num_items = int(info["n_users"]), int(info["n_items"])
        self.alpha, self.beta, self.k, self.band = alpha, beta, k, band
        try:
            self._check()
            rows = int(k)
        except (ValueError, TypeError):
            rows = 0                      # the refusal is raised by the first call that would use the tables
        self.nbr_w = nn.Parameter(torch.zeros(rows, self.num_items, dtype=torch.float32), requires_grad=False)
        self.register_buffer("nbr_id", torch.full((rows, self.num_items), -1, dtype=torch.int32))
        self.register_buffer("fitted", torch.zeros(1, dtype=torch.int32))
        self._csr = None                  # (device, rowptr, col, val) of the dataset's rating matrix

    # ------------------------------------------------------------------ the ratings
    def _check(self):
        check_config(self.alpha, self.beta, self.k, self.band, self.num_users)

    def _device(self):
        dev = self.nbr_w.device
        if dev.type != "cuda":
            raise _lib.HipCallError("RP3beta tables are on the CPU: call .to('cuda') first (no CPU fallback)")
        return dev

    def _ratings(self, dev):
        from ..defense.pca_select_users import rating_csr

        if self._csr is None or self._csr[0] != dev:
            U, I, rowptr, col, val = rating_csr(self.dataset, dev)
            if (U, I) != (self.num_users, self.num_items):
                raise ValueError(f"RP3beta: the dataset's rating matrix is {U} x {I}, its description says {self.num_users} x {self.num_items}")
            if col.numel() == 0:          # an empty matrix still needs addresses
                col, val = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.float32, device=dev)
            self._csr = (dev, rowptr, col, val)
        return self._csr[1:]

    @staticmethod
    def _validate(n_rows, n_cols, rowptr, col, val, what, dev):
        """rk_knn_norms; a refusal raises ValueError with the rule and the row, and nothing further is launched."""
        L, P = _lib.lib(), _lib.ptr
        rnorm = torch.empty(n_rows, dtype=torch.float32, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        rc = L.rk_knn_norms(n_rows, n_cols, P(rowptr), P(col), P(val), P(rnorm), P(status), _lib.stream_ptr(dev))
        if rc != 0:
            rule, row = status.cpu().tolist()
            if rule:
                raise ValueError(f"RP3beta: the {what} breaks rule {rule} ({_lib.RK_KNN_RULES.get(rule, '?')}), first in row {row}")
            _lib.check(rc, "rk_knn_norms")

    # ------------------------------------------------------------------ the fit
    def fit(self):
        """Builds the neighbour tables from the dataset's rating matrix, whether or not they were built before."""
        self._check()
        dev = self._device()
        _lib.require_gpu()
        U, I, k = self.num_users, self.num_items, int(self.k)
        alpha, beta = float(self.alpha), float(self.beta)
        rowptr, col, val = self._ratings(dev)
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
        nnz = int(col.numel())
        colptr = torch.empty(I + 1, dtype=torch.int32, device=dev)
        crow = torch.empty(nnz, dtype=torch.int32, device=dev)
        cval = torch.empty(nnz, dtype=torch.float32, device=dev)
        self._validate(U, I, rowptr, col, val, "rating matrix", dev)
        _lib.check(L.rk_pca_transpose(U, I, P(rowptr), P(col), P(val), P(colptr), P(crow), P(cval), s), "rk_pca_transpose")
        self._validate(I, U, colptr, crow, cval, "transposed rating matrix (rows are items)", dev)
        steps = torch.empty(nnz, dtype=torch.int64, device=dev)
        r = torch.empty(U, dtype=torch.int64, device=dev)
        fa, fb = torch.empty(I, dtype=torch.float64, device=dev), torch.empty(I, dtype=torch.float64, device=dev)
        _lib.check(L.rk_rp3_steps(U, P(rowptr), P(val), alpha, P(steps), P(r), s), "rk_rp3_steps")
        _lib.check(L.rk_rp3_factors(I, P(colptr), alpha, beta, P(fa), P(fb), s), "rk_rp3_factors")
        _lib.check(L.rk_rp3_neighbors(U, I, P(rowptr), P(col), P(steps), P(colptr), P(crow), P(fa), P(fb), k, int(self.band or 0), None,
                                      P(self.nbr_id), P(self.nbr_w.data), s), "rk_rp3_neighbors")
        self.fitted.fill_(1)
        self._known_fit = True
        return self

    _known_fit = None                     # what `fitted` holds, once it has been read back; None: not known

    def _fitted_tables(self):
        self._check()
        dev = self._device()
        if self._known_fit is None:
            self._known_fit = bool(self.fitted.item())
        if not self._known_fit:
            self.fit()
        return dev, self.nbr_id, self.nbr_w.data

    def _load_from_state_dict(self, *args, **kwargs):
        self._known_fit = None            # `fitted` is about to be overwritten
        return super()._load_from_state_dict(*args, **kwargs)

    def train_step(self, **config):
        """Fits on first use and is a no-op afterwards (workflow.normal_train calls it rec_epoch times).  The model has no loss:
        the value returned is 0.0."""
        self._fitted_tables()
        return (0.0,)

    # ------------------------------------------------------------------ scoring
    def forward(self, users, items):
        dev, nbr_id, nbr_w = self._fitted_tables()
        rowptr, col, val = self._ratings(dev)
        users, items = users.long().contiguous(), items.long().contiguous()
        n = users.numel()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().rk_rp3_pair_scores(
            self.num_items, self.num_users, int(self.k), _lib.ptr(nbr_id), _lib.ptr(nbr_w), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val),
            _lib.ptr(users) if n else None, _lib.ptr(items) if n else None, n, _lib.ptr(out) if n else None,
            _lib.stream_ptr(dev)), "rk_rp3_pair_scores")
        return out

    def score_matrix(self, user_ids, out):
        """out[len(user_ids), n_items] <- the score of every item for each user (int32 ids on the device), seen items included;
        the batched evaluation then runs rk_topk_rows on it."""
        dev, nbr_id, nbr_w = self._fitted_tables()
        rowptr, col, val = self._ratings(dev)
        _lib.check(_lib.lib().rk_rp3_scores(
            self.num_users, self.num_items, int(self.k), _lib.ptr(nbr_id), _lib.ptr(nbr_w), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val),
            user_ids.numel(), _lib.ptr(user_ids), int(self.band or 0), _lib.ptr(out), _lib.stream_ptr(dev)), "rk_rp3_scores")

    def input_describe(self):
        return {
            "train_step": {},
            "forward": {"users": (torch.int64, (VarDim(comment="batch"))), "items": (torch.int64, (VarDim(comment="batch")))},
        }

    def output_describe(self):
        return {
            "train_step": {"loss": (float, [])},   # always 0.0: the model has no loss
            "forward": {"unnormalized_scores": (torch.float32, [VarDim(comment="batch")])},
        }
