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
from .._ratings import checked_norms, device_refusal, transposed
from ._fit_once import FitOnceVictim, matrix_score_pairs, matrix_score_rows


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


class SLIM(FitOnceVictim):
    victim_name = "slim"
    label, state_noun = "SLIM", "weights"

    def _build(self, l1_reg, l2_reg, sweeps, **config):
        self._open(config)
        self.l1_reg, self.l2_reg, self.sweeps = l1_reg, l2_reg, sweeps
        rows = self.num_items if self._accepted() else 0
        self.W = nn.Parameter(torch.zeros(rows, rows, dtype=torch.float32), requires_grad=False)
        self.register_buffer("fitted", torch.zeros(1, dtype=torch.int32))
        self._info = None                 # int32 [I, 3] of the last fit this object ran

    def _check(self):
        check_config(self.l1_reg, self.l2_reg, self.sweeps)
        if not 1 <= self.num_items <= _lib.RK_SLIM_MAX_ITEMS:
            raise ValueError(f"SLIM: {self.num_items} items, a column's residual and weights live in one workgroup's LDS, which holds a "
                             f"catalogue of 1..{_lib.RK_SLIM_MAX_ITEMS} at most (the yelp-shaped catalogue is out of reach)")

    # ------------------------------------------------------------------ the fit
    def _fit(self, dev, rowptr, col, val):
        """Builds W from the rating matrix.  A device refusal names the rule and the row or item, and leaves the model unfitted:
        the columns are descended inside W's own storage, so `fitted` is cleared first."""
        U, I = self.num_users, self.num_items
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
        self._unfit()
        self._info = None
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        checked_norms("SLIM", "rating matrix", U, I, rowptr, col, val)                  # rules 1, 2, 3, 4
        colptr, crow, cval = transposed(U, I, rowptr, col, val)
        G = torch.empty(I * I, dtype=torch.float32, device=dev)       # the fit's temporary: the second I x I matrix
        bad = device_refusal(L.rk_ease_gram(U, I, P(rowptr), P(col), P(val), P(colptr), P(crow), P(cval), float(self.l2_reg), P(G),
                                            P(status), s), "rk_ease_gram", status)
        if bad:
            raise ValueError(f"SLIM: the rating matrix breaks rule {bad[0]} (an item's squared norm of 2^24 or more), first in item {bad[1]}")
        info = torch.empty(I, 3, dtype=torch.int32, device=dev)
        bad = device_refusal(L.rk_slim_fit(I, P(G), float(self.l1_reg), int(self.sweeps), P(self.W.data), P(info), None, P(status), s),
                             "rk_slim_fit", status)
        if bad:
            raise ValueError(f"SLIM: rule {bad[0]} (a diagonal entry of the regularised Gram matrix is not a finite number > 0), at item {bad[1]}")
        self._info = info

    def fit_info(self):
        """Per column (int32 [I] each, on the device): the last sweep that changed a coordinate (0: none did), the number of
        positive weights, and the number of coordinate steps that changed a weight.  The diagnostics belong to a fit this object
        ran: a model that is unfitted, or whose weights were loaded, is fitted first (the same bits)."""
        self._fitted()
        if self._info is None:
            self.fit()
        last, support, steps = self._info.unbind(dim=1)
        return {"last_sweep": last, "support": support, "steps": steps}

    # ------------------------------------------------------------------ scoring
    def _score_pairs(self, csr, users, items, n, out, stream):
        matrix_score_pairs(self.W.data, self.num_items, self.num_users, csr, users, items, n, out, stream)

    def _score_rows(self, csr, user_ids, out, stream):
        matrix_score_rows(self.W.data, self.num_items, csr, user_ids, out, stream)
