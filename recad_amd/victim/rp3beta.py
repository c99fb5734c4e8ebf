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
from .._ratings import checked_norms, transposed
from ._fit_once import FitOnceVictim


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


class RP3beta(FitOnceVictim):
    victim_name = "rp3beta"
    label, state_noun = "RP3beta", "tables"

    def _build(self, alpha, beta, k, band, **config):
        self._open(config)
        self.alpha, self.beta, self.k, self.band = alpha, beta, k, band
        rows = int(k) if self._accepted() else 0
        self.nbr_w = nn.Parameter(torch.zeros(rows, self.num_items, dtype=torch.float32), requires_grad=False)
        self.register_buffer("nbr_id", torch.full((rows, self.num_items), -1, dtype=torch.int32))
        self.register_buffer("fitted", torch.zeros(1, dtype=torch.int32))

    def _check(self):
        check_config(self.alpha, self.beta, self.k, self.band, self.num_users)

    # ------------------------------------------------------------------ the fit
    def _fit(self, dev, rowptr, col, val):
        """Builds the neighbour tables from the rating matrix."""
        U, I = self.num_users, self.num_items
        alpha, beta = float(self.alpha), float(self.beta)
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
        checked_norms("RP3beta", "rating matrix", U, I, rowptr, col, val)
        colptr, crow, cval = transposed(U, I, rowptr, col, val)
        checked_norms("RP3beta", "transposed rating matrix (rows are items)", I, U, colptr, crow, cval)
        steps = torch.empty(col.numel(), dtype=torch.int64, device=dev)
        r = torch.empty(U, dtype=torch.int64, device=dev)
        fa, fb = torch.empty(I, dtype=torch.float64, device=dev), torch.empty(I, dtype=torch.float64, device=dev)
        _lib.check(L.rk_rp3_steps(U, P(rowptr), P(val), alpha, P(steps), P(r), s), "rk_rp3_steps")
        _lib.check(L.rk_rp3_factors(I, P(colptr), alpha, beta, P(fa), P(fb), s), "rk_rp3_factors")
        _lib.check(L.rk_rp3_neighbors(U, I, P(rowptr), P(col), P(steps), P(colptr), P(crow), P(fa), P(fb), int(self.k),
                                      int(self.band or 0), None, P(self.nbr_id), P(self.nbr_w.data), s), "rk_rp3_neighbors")

    # ------------------------------------------------------------------ scoring
    def _score_pairs(self, csr, users, items, n, out, stream):
        P = _lib.ptr
        _lib.check(_lib.lib().rk_rp3_pair_scores(self.num_items, self.num_users, int(self.k), P(self.nbr_id), P(self.nbr_w.data),
                                                 *map(P, csr), users, items, n, out, stream), "rk_rp3_pair_scores")

    def _score_rows(self, csr, user_ids, out, stream):
        P = _lib.ptr
        _lib.check(_lib.lib().rk_rp3_scores(self.num_users, self.num_items, int(self.k), P(self.nbr_id), P(self.nbr_w.data), *map(P, csr),
                                            user_ids.numel(), P(user_ids), int(self.band or 0), P(out), stream), "rk_rp3_scores")
