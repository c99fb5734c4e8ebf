"""UserKNN victim on MI355X: user-neighbourhood collaborative filtering (Resnick et al. 1994; Breese et al. 1998; Herlocker et al.
1999), the recommender the shilling literature was written against (Lam and Riedl 2004; Mobasher et al. 2007): the average,
segment and bandwagon profiles are built so that the fake users become neighbours of real ones.  Its similarity is the user-user
cosine of the ``KnnSelectUsers`` defender, so the kept weights of a user are that defender's ``topw``, bit for bit.

It is not in the reference, whose victims are all trained embedding models.  include/recad_hip.h states the exact definition
(integer co-rating dots, fp32 cosine weights in a fixed operation order, neighbours by (w descending, id ascending), the sum in
slot order, and with ``normalize`` the weighted average over the neighbours who rated the item), csrc/userknn.hip scores it by
gathering whole neighbour rows into a catalogue row in LDS, and tests/_userknn_restate.py restates it in numpy, bit for bit.  The
neighbour tables come from rk_itemknn_neighbors pointed at the other side of the matrix; there is no second neighbour kernel.

``normalize=True`` on implicit data is degenerate by definition (every reachable item scores exactly 1.0); it is meant for
ratings.  Not built: mean-centring, significance weighting, shrinkage.

Like ``ItemKNN`` it has no sampler, no initialisation and no epochs: ``train_step`` builds the tables on first use and does
nothing afterwards.  The tables are module state (``nbr_w`` a frozen parameter ``[k, U]``, ``nbr_id`` and ``fitted`` buffers)."""
import torch
import torch.nn as nn

from .. import _lib
from .._ratings import checked_norms, transposed
from ._fit_once import FitOnceVictim


def check_config(k, normalize, band):
    """The host-side refusals (ValueError), before any device call."""
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= _lib.RK_KNN_MAX_K:
        raise ValueError(f"UserKNN: k = {k!r} outside 1..{_lib.RK_KNN_MAX_K}")
    if not isinstance(normalize, bool):
        raise ValueError(f"UserKNN: normalize = {normalize!r}, expected True or False")
    if band is not None and (isinstance(band, bool) or int(band) != band or band % 64 or not 64 <= band <= _lib.RK_USERKNN_MAX_BAND):
        raise ValueError(f"UserKNN: band = {band!r}, expected None or a multiple of 64 in 64..{_lib.RK_USERKNN_MAX_BAND}")


class UserKNN(FitOnceVictim):
    victim_name = "userknn"
    label, state_noun = "UserKNN", "tables"

    def _build(self, k, normalize, band, **config):
        self._open(config)
        self.k, self.normalize, self.band = k, normalize, band
        rows = int(k) if self._accepted() else 0
        self.nbr_w = nn.Parameter(torch.zeros(rows, self.num_users, dtype=torch.float32), requires_grad=False)
        self.register_buffer("nbr_id", torch.full((rows, self.num_users), -1, dtype=torch.int32))
        self.register_buffer("fitted", torch.zeros(1, dtype=torch.int32))

    def _check(self):
        check_config(self.k, self.normalize, self.band)

    # ------------------------------------------------------------------ the fit
    def _fit(self, dev, rowptr, col, val):
        """Builds the neighbour tables from the rating matrix: rk_itemknn_neighbors on the transposed roles."""
        U, I = self.num_users, self.num_items
        L, P = _lib.lib(), _lib.ptr
        rnorm_user = checked_norms("UserKNN", "rating matrix", U, I, rowptr, col, val)                  # r_u, rules 1 to 4
        colptr, crow, cval = transposed(U, I, rowptr, col, val)
        checked_norms("UserKNN", "transposed rating matrix (rows are items)", I, U, colptr, crow, cval)   # rule 3 for the columns
        # the fit band is the neighbour kernel's own automatic one: `band` is the scoring kernel's
        _lib.check(L.rk_itemknn_neighbors(I, U, P(colptr), P(crow), P(cval), P(rowptr), P(col), P(val), P(rnorm_user), int(self.k),
                                          0, None, P(self.nbr_id), P(self.nbr_w.data), _lib.stream_ptr(dev)),
                   "rk_itemknn_neighbors")

    # ------------------------------------------------------------------ scoring
    def _score_pairs(self, csr, users, items, n, out, stream):
        P = _lib.ptr
        _lib.check(_lib.lib().rk_userknn_pair_scores(self.num_items, self.num_users, int(self.k), P(self.nbr_id), P(self.nbr_w.data),
                                                     *map(P, csr), users, items, n, int(self.normalize), out, stream),
                   "rk_userknn_pair_scores")

    def _score_rows(self, csr, user_ids, out, stream):
        P = _lib.ptr
        _lib.check(_lib.lib().rk_userknn_scores(self.num_users, self.num_items, int(self.k), P(self.nbr_id), P(self.nbr_w.data),
                                                *map(P, csr), user_ids.numel(), P(user_ids), int(self.normalize), int(self.band or 0),
                                                P(out), stream), "rk_userknn_scores")
