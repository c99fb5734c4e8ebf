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
from ..utils import VarDim
from .base import BaseVictim

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


class EASE(BaseVictim):
    victim_name = "ease"

    def _build(self, reg_lambda, block, **config):
        self.dataset = config["dataset"]
        self.config = config
        info = self.dataset.info_describe()
        self.num_users, self.num_items = int(info["n_users"]), int(info["n_items"])
        self.reg_lambda, self.block = reg_lambda, block
        try:
            self._check()
            rows = self.num_items
        except (ValueError, TypeError):
            rows = 0                      # the refusal is raised by the first call that would use B
        self.B = nn.Parameter(torch.zeros(rows, rows, dtype=torch.float32), requires_grad=False)
        self.register_buffer("fitted", torch.zeros(1, dtype=torch.int32))
        self._csr = None                  # (device, rowptr, col, val) of the dataset's rating matrix

    # ------------------------------------------------------------------ the ratings
    def _check(self):
        check_config(self.reg_lambda, self.block)
        if not 1 <= self.num_items <= _lib.RK_EASE_MAX_ITEMS:
            raise ValueError(f"EASE: {self.num_items} items, the item-item matrix holds a catalogue of 1..{_lib.RK_EASE_MAX_ITEMS} at most")

    def _device(self):
        dev = self.B.device
        if dev.type != "cuda":
            raise _lib.HipCallError("EASE weights are on the CPU: call .to('cuda') first (no CPU fallback)")
        return dev

    def _ratings(self, dev):
        from ..defense.pca_select_users import rating_csr

        if self._csr is None or self._csr[0] != dev:
            U, I, rowptr, col, val = rating_csr(self.dataset, dev)
            if (U, I) != (self.num_users, self.num_items):
                raise ValueError(f"EASE: the dataset's rating matrix is {U} x {I}, its description says {self.num_users} x {self.num_items}")
            if col.numel() == 0:          # an empty matrix still needs addresses
                col, val = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.float32, device=dev)
            self._csr = (dev, rowptr, col, val)
        return self._csr[1:]

    # ------------------------------------------------------------------ the fit
    def fit(self):
        """Builds B from the dataset's rating matrix, whether or not it was built before.  A device refusal raises ValueError
        with the rule and the row, item or pivot, and leaves the model unfitted."""
        self._check()
        dev = self._device()
        _lib.require_gpu()
        U, I = self.num_users, self.num_items
        rowptr, col, val = self._ratings(dev)
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
        self.fitted.zero_()
        self._known_fit = False
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
            raise ValueError(f"EASE: the rating matrix breaks rule {bad[0]} ({_lib.RK_KNN_RULES.get(bad[0], '?')}), first in row {bad[1]}")
        _lib.check(L.rk_pca_transpose(U, I, P(rowptr), P(col), P(val), P(colptr), P(crow), P(cval), s), "rk_pca_transpose")
        A = self.B.data
        bad = refused(L.rk_ease_gram(U, I, P(rowptr), P(col), P(val), P(colptr), P(crow), P(cval), float(self.reg_lambda), P(A), P(status), s),
                      "rk_ease_gram")
        if bad:
            raise ValueError(f"EASE: the rating matrix breaks rule {bad[0]} (an item's squared norm of 2^24 or more), first in item {bad[1]}")
        b = resolved_block(I, self.block)
        work = torch.empty(I * b, dtype=torch.float32, device=dev)
        bad = refused(L.rk_ease_invert(I, P(A), P(work), work.numel(), int(self.block or 0), P(status), s), "rk_ease_invert")
        if bad:
            raise ValueError(f"EASE: rule {bad[0]} (the regularised Gram matrix is not positive definite in fp32), at pivot {bad[1]}")
        _lib.check(L.rk_ease_weights(I, P(A), P(A), s), "rk_ease_weights")
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
        return dev, self.B.data

    def _load_from_state_dict(self, *args, **kwargs):
        self._known_fit = None            # `fitted` is about to be overwritten
        return super()._load_from_state_dict(*args, **kwargs)

    def train_step(self, **config):
        """Fits on first use and is a no-op afterwards (workflow.normal_train calls it rec_epoch times).  A closed-form model
        has no loss: the value returned is 0.0."""
        self._fitted_weights()
        return (0.0,)

    # ------------------------------------------------------------------ scoring
    def forward(self, users, items):
        dev, B = self._fitted_weights()
        rowptr, col, val = self._ratings(dev)
        users, items = users.long().contiguous(), items.long().contiguous()
        n = users.numel()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().rk_ease_pair_scores(
            self.num_items, self.num_users, _lib.ptr(B), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val),
            _lib.ptr(users) if n else None, _lib.ptr(items) if n else None, n, _lib.ptr(out) if n else None, _lib.stream_ptr(dev)),
            "rk_ease_pair_scores")
        return out

    def score_matrix(self, user_ids, out):
        """out[len(user_ids), n_items] <- the score of every item for each user (int32 ids on the device), seen items included;
        the batched evaluation then runs rk_topk_rows on it."""
        dev, B = self._fitted_weights()
        rowptr, col, val = self._ratings(dev)
        _lib.check(_lib.lib().rk_ease_scores(
            self.num_items, _lib.ptr(B), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), user_ids.numel(), _lib.ptr(user_ids), _lib.ptr(out),
            _lib.stream_ptr(dev)), "rk_ease_scores")

    def input_describe(self):
        return {
            "train_step": {},
            "forward": {"users": (torch.int64, (VarDim(comment="batch"))), "items": (torch.int64, (VarDim(comment="batch")))},
        }

    def output_describe(self):
        return {
            "train_step": {"loss": (float, [])},   # always 0.0: a closed-form model has no loss
            "forward": {"unnormalized_scores": (torch.float32, [VarDim(comment="batch")])},
        }
