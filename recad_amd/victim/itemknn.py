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
from .._ratings import checked_norms, transposed
from ._fit_once import FitOnceVictim


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


class ItemKNN(FitOnceVictim):
    victim_name = "itemknn"
    label, state_noun = "ItemKNN", "tables"

    def _build(self, k, band, user_block, **config):
        self._open(config)
        self.k, self.band, self.user_block = k, band, user_block
        # by check_config alone, not _check: a catalogue the scoring kernel cannot hold keeps its k table rows, as it always has
        rows = int(k) if self._accepted(lambda: check_config(k, band, user_block)) else 0
        self.nbr_w = nn.Parameter(torch.zeros(rows, self.num_items, dtype=torch.float32), requires_grad=False)
        self.register_buffer("nbr_id", torch.full((rows, self.num_items), -1, dtype=torch.int32))
        self.register_buffer("fitted", torch.zeros(1, dtype=torch.int32))

    def _check(self):
        check_config(self.k, self.band, self.user_block)
        if self.num_items > _lib.RK_ITEMKNN_MAX_ITEMS:
            raise ValueError(f"ItemKNN: {self.num_items} items, the scoring kernel holds a catalogue of at most {_lib.RK_ITEMKNN_MAX_ITEMS}")
        if self.user_block is not None and self.user_block > rows_that_fit(self.num_items):
            raise ValueError(f"ItemKNN: user_block = {self.user_block}, only {rows_that_fit(self.num_items)} byte rows of "
                             f"{self.num_items} items fit a CU's LDS")

    # ------------------------------------------------------------------ the fit
    def _fit(self, dev, rowptr, col, val):
        """Builds the neighbour tables from the rating matrix."""
        U, I = self.num_users, self.num_items
        L, P = _lib.lib(), _lib.ptr
        checked_norms("ItemKNN", "rating matrix", U, I, rowptr, col, val)               # rules 1, 2, 4 (and the user norms' rule 3)
        colptr, crow, cval = transposed(U, I, rowptr, col, val)
        rnorm_item = checked_norms("ItemKNN", "transposed rating matrix (rows are items)", I, U, colptr, crow, cval)   # r_i, rule 3
        _lib.check(L.rk_itemknn_neighbors(U, I, P(rowptr), P(col), P(val), P(colptr), P(crow), P(cval), P(rnorm_item), int(self.k),
                                          int(self.band or 0), None, P(self.nbr_id), P(self.nbr_w.data), _lib.stream_ptr(dev)),
                   "rk_itemknn_neighbors")

    # ------------------------------------------------------------------ scoring
    def _score_pairs(self, csr, users, items, n, out, stream):
        P = _lib.ptr
        _lib.check(_lib.lib().rk_itemknn_pair_scores(self.num_items, self.num_users, int(self.k), P(self.nbr_id), P(self.nbr_w.data),
                                                     *map(P, csr), users, items, n, out, stream), "rk_itemknn_pair_scores")

    def _score_rows(self, csr, user_ids, out, stream):
        P = _lib.ptr
        _lib.check(_lib.lib().rk_itemknn_scores(self.num_items, int(self.k), P(self.nbr_id), P(self.nbr_w.data), *map(P, csr),
                                                user_ids.numel(), P(user_ids), int(self.user_block or 0), P(out), stream), "rk_itemknn_scores")
