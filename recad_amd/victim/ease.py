"""EASE victim on MI355X: the linear item-item autoencoder with a closed-form fit (Steck 2019, "Embarrassingly Shallow
Autoencoders for Sparse Data"): P = (X^T X + lambda I)^-1, B_ij = -P_ij / P_jj off the diagonal, score(u, .) = x_u B.

It is not in the reference, whose victims are all trained embedding models.  include/recad_hip.h states the exact definition
(an integer Gram matrix, the fp32 inverse under an error budget, weights by one double division, scores as an fp32 chain in
column order), csrc/ease.hip computes it with a hand-written blocked Gauss-Jordan inverse, and tests/_ease_restate.py restates
it in numpy.  The fit has no sampler, no initialisation and no epoch count: two fits of the same data give the same bits.

"Training" is the fit: ``train_step`` builds B on first use and does nothing afterwards.  ``B`` is a frozen parameter and
``fitted`` a buffer, so ``.to()``, ``state_dict()`` and ``next(victim.parameters()).device`` behave as for the trained victims.
P is inverted inside B's own storage: no second I x I matrix is kept.  The ratings themselves come from the dataset."""
import math

import torch
import torch.nn as nn

from .. import _lib
from .._ratings import checked_norms, device_refusal, transposed
from ._fit_once import FitOnceVictim, matrix_score_pairs, matrix_score_rows

_BLOCKS = (_lib.RK_EASE_BLOCK_SMALL, _lib.RK_EASE_BLOCK_LARGE)


def check_config(reg_lambda, block):
    """The host-side refusals (ValueError), before any device call."""
    ok = not isinstance(reg_lambda, bool) and isinstance(reg_lambda, (int, float))
    if ok:
        as_f32 = torch.tensor(float(reg_lambda), dtype=torch.float32).item()       # what the kernel receives
        ok = math.isfinite(as_f32) and as_f32 > 0
    if not ok:
        raise ValueError(f"EASE: reg_lambda = {reg_lambda!r}, expected a finite fp32 number > 0")
    if block is not None and (isinstance(block, bool) or block not in _BLOCKS):
        raise ValueError(f"EASE: block = {block!r}, expected None, {_BLOCKS[0]} or {_BLOCKS[1]}")


def resolved_block(n_items, block):
    """The block width rk_ease_invert uses: its workspace is n_items * resolved_block floats."""
    return int(block) if block else (_BLOCKS[0] if n_items <= _BLOCKS[0] else _BLOCKS[1])


class EASE(FitOnceVictim):
    victim_name = "ease"
    label, state_noun = "EASE", "weights"

    def _build(self, reg_lambda, block, **config):
        self._open(config)
        self.reg_lambda, self.block = reg_lambda, block
        rows = self.num_items if self._accepted() else 0
        self.B = nn.Parameter(torch.zeros(rows, rows, dtype=torch.float32), requires_grad=False)
        self.register_buffer("fitted", torch.zeros(1, dtype=torch.int32))

    def _check(self):
        check_config(self.reg_lambda, self.block)
        if not 1 <= self.num_items <= _lib.RK_EASE_MAX_ITEMS:
            raise ValueError(f"EASE: {self.num_items} items, the item-item matrix holds a catalogue of 1..{_lib.RK_EASE_MAX_ITEMS} at most")

    # ------------------------------------------------------------------ the fit
    def _fit(self, dev, rowptr, col, val):
        """Builds B from the rating matrix.  A device refusal names the rule and the row, item or pivot, and leaves the model
        unfitted: the inverse is formed inside B's own storage, so `fitted` is cleared first."""
        U, I = self.num_users, self.num_items
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
        self._unfit()
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        checked_norms("EASE", "rating matrix", U, I, rowptr, col, val)                  # rules 1, 2, 3, 4
        colptr, crow, cval = transposed(U, I, rowptr, col, val)
        A = self.B.data
        bad = device_refusal(L.rk_ease_gram(U, I, P(rowptr), P(col), P(val), P(colptr), P(crow), P(cval), float(self.reg_lambda), P(A),
                                            P(status), s), "rk_ease_gram", status)
        if bad:
            raise ValueError(f"EASE: the rating matrix breaks rule {bad[0]} (an item's squared norm of 2^24 or more), first in item {bad[1]}")
        b = resolved_block(I, self.block)
        work = torch.empty(I * b, dtype=torch.float32, device=dev)
        bad = device_refusal(L.rk_ease_invert(I, P(A), P(work), work.numel(), int(self.block or 0), P(status), s), "rk_ease_invert", status)
        if bad:
            raise ValueError(f"EASE: rule {bad[0]} (the regularised Gram matrix is not positive definite in fp32), at pivot {bad[1]}")
        _lib.check(L.rk_ease_weights(I, P(A), P(A), s), "rk_ease_weights")

    # ------------------------------------------------------------------ scoring
    def _score_pairs(self, csr, users, items, n, out, stream):
        matrix_score_pairs(self.B.data, self.num_items, self.num_users, csr, users, items, n, out, stream)

    def _score_rows(self, csr, user_ids, out, stream):
        matrix_score_rows(self.B.data, self.num_items, csr, user_ids, out, stream)
