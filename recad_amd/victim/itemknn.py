"""ItemKNN victim on MI355X: item-neighbourhood collaborative filtering (Sarwar et al. 2001; Deshpande and Karypis 2004), the
memory-based recommender the heuristic attackers (random, average, segment, bandwagon) were designed against.

It is not in the reference, whose victims are all trained embedding models.  include/recad_hip.h states the exact definition
(integer co-rating dots, fp32 cosine weights in a fixed operation order, neighbours by (w descending, id ascending), the
un-normalised sum in slot order), csrc/itemknn.hip computes it without an I x I matrix, and tests/_itemknn_restate.py restates
it in numpy, bit for bit.

"Training" is the fit: ``train_step`` builds the neighbour tables on first use and does nothing afterwards.  The tables are
module state (``nbr_w`` a frozen parameter, ``nbr_id`` and ``fitted`` buffers), so ``.to()``, ``state_dict()`` and
``next(victim.parameters()).device`` behave as for the trained victims.  The ratings themselves come from the dataset."""
import torch
import torch.nn as nn

from .. import _lib
from ..utils import VarDim
from .base import BaseVictim


def check_config(k, band, user_block):
    """The host-side refusals (ValueError), before any device call."""
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= _lib.RK_KNN_MAX_K:
        raise ValueError(f"ItemKNN: k = {k!r} outside 1..{_lib.RK_KNN_MAX_K}")
    if band is not None and (isinstance(band, bool) or int(band) != band or band % 64 or not 64 <= band <= _lib.RK_ITEMKNN_MAX_BAND):
        raise ValueError(f"ItemKNN: band = {band!r}, expected None or a multiple of 64 in 64..{_lib.RK_ITEMKNN_MAX_BAND}")
    if user_block is not None and (isinstance(user_block, bool) or int(user_block) != user_block
                                   or not 1 <= user_block <= _lib.RK_ITEMKNN_MAX_USER_BLOCK):
        raise ValueError(f"ItemKNN: user_block = {user_block!r}, expected None or 1..{_lib.RK_ITEMKNN_MAX_USER_BLOCK}")


def rows_that_fit(n_items):
    """How many users' byte rows of an n_items catalogue one workgroup of rk_itemknn_scores can hold (0: none)."""
    return _lib.RK_ITEMKNN_MAX_ITEMS // ((int(n_items) + 15) // 16 * 16)


class ItemKNN(BaseVictim):
    victim_name = "itemknn"

    def _build(self, k, band, user_block, **config):
        self.dataset = config["dataset"]
        self.config = config
        info = self.dataset.info_describe()
        self.num_users, self.num_items = int(info["n_users"]), int(info["n_items"])
        self.k, self.band, self.user_block = k, band, user_block
        try:
            check_config(k, band, user_block)
            rows = int(k)
        except (ValueError, TypeError):
            rows = 0                      # the refusal is raised by the first call that would use the tables
        self.nbr_w = nn.Parameter(torch.zeros(rows, self.num_items, dtype=torch.float32), requires_grad=False)
        self.register_buffer("nbr_id", torch.full((rows, self.num_items), -1, dtype=torch.int32))
        self.register_buffer("fitted", torch.zeros(1, dtype=torch.int32))
        self._csr = None                  # (device, rowptr, col, val) of the dataset's rating matrix

    # ------------------------------------------------------------------ the ratings
    def _check(self):
        check_config(self.k, self.band, self.user_block)
        if self.num_items > _lib.RK_ITEMKNN_MAX_ITEMS:
            raise ValueError(f"ItemKNN: {self.num_items} items, the scoring kernel holds a catalogue of at most {_lib.RK_ITEMKNN_MAX_ITEMS}")
        if self.user_block is not None and self.user_block > rows_that_fit(self.num_items):
            raise ValueError(f"ItemKNN: user_block = {self.user_block}, only {rows_that_fit(self.num_items)} byte rows of "
                             f"{self.num_items} items fit a CU's LDS")

    def _device(self):
        dev = self.nbr_w.device
        if dev.type != "cuda":
            raise _lib.HipCallError("ItemKNN tables are on the CPU: call .to('cuda') first (no CPU fallback)")
        return dev

    def _ratings(self, dev):
        from ..defense.pca_select_users import rating_csr

        if self._csr is None or self._csr[0] != dev:
            U, I, rowptr, col, val = rating_csr(self.dataset, dev)
            if (U, I) != (self.num_users, self.num_items):
                raise ValueError(f"ItemKNN: the dataset's rating matrix is {U} x {I}, its description says {self.num_users} x {self.num_items}")
            if col.numel() == 0:          # an empty matrix still needs addresses
                col, val = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.float32, device=dev)
            self._csr = (dev, rowptr, col, val)
        return self._csr[1:]

    @staticmethod
    def _norms(n_rows, n_cols, rowptr, col, val, what, dev):
        """rk_knn_norms; a refusal raises ValueError with the rule and the row, and nothing further is launched."""
        L, P = _lib.lib(), _lib.ptr
        rnorm = torch.empty(n_rows, dtype=torch.float32, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        rc = L.rk_knn_norms(n_rows, n_cols, P(rowptr), P(col), P(val), P(rnorm), P(status), _lib.stream_ptr(dev))
        if rc != 0:
            rule, row = status.cpu().tolist()
            if rule:
                raise ValueError(f"ItemKNN: the {what} breaks rule {rule} ({_lib.RK_KNN_RULES.get(rule, '?')}), first in row {row}")
            _lib.check(rc, "rk_knn_norms")
        return rnorm

    # ------------------------------------------------------------------ the fit
    def fit(self):
        """Builds the neighbour tables from the dataset's rating matrix, whether or not they were built before."""
        self._check()
        dev = self._device()
        _lib.require_gpu()
        U, I, k = self.num_users, self.num_items, int(self.k)
        rowptr, col, val = self._ratings(dev)
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
        nnz = int(col.numel())
        colptr = torch.empty(I + 1, dtype=torch.int32, device=dev)
        crow = torch.empty(nnz, dtype=torch.int32, device=dev)
        cval = torch.empty(nnz, dtype=torch.float32, device=dev)
        self._norms(U, I, rowptr, col, val, "rating matrix", dev)                       # rules 1, 2, 4 (and the user norms' rule 3)
        _lib.check(L.rk_pca_transpose(U, I, P(rowptr), P(col), P(val), P(colptr), P(crow), P(cval), s), "rk_pca_transpose")
        rnorm_item = self._norms(I, U, colptr, crow, cval, "transposed rating matrix (rows are items)", dev)   # r_i, rule 3
        _lib.check(L.rk_itemknn_neighbors(U, I, P(rowptr), P(col), P(val), P(colptr), P(crow), P(cval), P(rnorm_item), k,
                                          int(self.band or 0), None, P(self.nbr_id), P(self.nbr_w.data), s), "rk_itemknn_neighbors")
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
        """Fits on first use and is a no-op afterwards (workflow.normal_train calls it rec_epoch times).  A memory-based model
        has no loss: the value returned is 0.0."""
        self._fitted_tables()
        return (0.0,)

    # ------------------------------------------------------------------ scoring
    def forward(self, users, items):
        dev, nbr_id, nbr_w = self._fitted_tables()
        rowptr, col, val = self._ratings(dev)
        users, items = users.long().contiguous(), items.long().contiguous()
        out = torch.empty(users.numel(), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().rk_itemknn_pair_scores(
            self.num_items, self.num_users, int(self.k), _lib.ptr(nbr_id), _lib.ptr(nbr_w), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val),
            _lib.ptr(users) if users.numel() else None, _lib.ptr(items) if users.numel() else None, users.numel(), _lib.ptr(out) if users.numel() else None,
            _lib.stream_ptr(dev)), "rk_itemknn_pair_scores")
        return out

    def score_matrix(self, user_ids, out):
        """out[len(user_ids), n_items] <- the score of every item for each user (int32 ids on the device), seen items included;
        the batched evaluation then runs rk_topk_rows on it."""
        dev, nbr_id, nbr_w = self._fitted_tables()
        rowptr, col, val = self._ratings(dev)
        _lib.check(_lib.lib().rk_itemknn_scores(
            self.num_items, int(self.k), _lib.ptr(nbr_id), _lib.ptr(nbr_w), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val),
            user_ids.numel(), _lib.ptr(user_ids), int(self.user_block or 0), _lib.ptr(out), _lib.stream_ptr(dev)), "rk_itemknn_scores")

    def input_describe(self):
        return {
            "train_step": {},
            "forward": {"users": (torch.int64, (VarDim(comment="batch"))), "items": (torch.int64, (VarDim(comment="batch")))},
        }

    def output_describe(self):
        return {
            "train_step": {"loss": (float, [])},   # always 0.0: a memory-based model has no loss
            "forward": {"unnormalized_scores": (torch.float32, [VarDim(comment="batch")])},
        }
