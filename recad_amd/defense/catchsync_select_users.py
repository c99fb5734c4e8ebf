"""CatchSyncSelectUsers: structure-only fake-user detection on the device.

CatchSync (Jiang, Cui, Beutel, Faloutsos, Yang, KDD 2014): users whose items sit close together in a feature space of the
items (synchronicity) and away from where most items sit (low normality) behave in lockstep.  Here the item features are the
degree and the reach (one HITS step from the all-ones hub vector), bucketed on a log grid by shifts and masks; the cells are
the distinct bucket pairs.  include/recad_hip.h states the exact definition (integers end to end, fp64 scores in a fixed
operation order), csrc/catchsync.hip computes it, tests/_catchsync_restate.py restates it in numpy, word for word.  It is not
in the reference, whose only defender is the spectral PCASelectUsers.

The ``flag_count(attack_num, U)`` users of LARGEST score are flagged.  ``score="sync"`` (default) is the share of a user's
distinct item pairs that fall into one cell, ``"normality"`` the mean share of all rated items in the cells of the user's
items, ``"residual"`` the synchronicity above the least one possible at the user's normality.  Users with fewer than
``min_items`` items score -1.  Not built: the converged HITS authority as second feature, the paper's per-bin 3-sigma rule,
scoring items.  DESIGN.md section 17 has the counts on synthetic data; nobody has measured real data."""
import numpy as np
import torch

from .. import _lib
from .._ratings import checked_norms, device_refusal, transposed
from ._select_users import SelectUsersDefender

SCORES = ("sync", "normality", "residual")
SCHEDULES = ("work", "natural")
FORMS = (None, "wave", "workgroup")


def check_config(score, grid_bits, min_items, schedule, form):
    """The host-side refusals (ValueError), before any device call."""
    if score not in SCORES:
        raise ValueError(f"CatchSyncSelectUsers: score = {score!r}, expected one of {SCORES}")
    if isinstance(grid_bits, bool) or not isinstance(grid_bits, (int, np.integer)) or not 0 <= grid_bits <= 3:
        raise ValueError(f"CatchSyncSelectUsers: grid_bits = {grid_bits!r}, expected an integer in 0..3")
    if isinstance(min_items, bool) or not isinstance(min_items, (int, np.integer)) or min_items < 2:
        raise ValueError(f"CatchSyncSelectUsers: min_items = {min_items!r}, expected an integer >= 2")
    if schedule not in SCHEDULES:
        raise ValueError(f"CatchSyncSelectUsers: schedule = {schedule!r}, expected one of {SCHEDULES}")
    if form not in FORMS:
        raise ValueError(f"CatchSyncSelectUsers: form = {form!r}, expected one of {FORMS}")


def work_order(rowptr):
    """Users by descending row length, ties to the lower id: int32 [U] on the device."""
    return torch.sort(rowptr[1:] - rowptr[:-1], descending=True, stable=True).indices.to(torch.int32).contiguous()


class CatchSyncSelectUsers(SelectUsersDefender):
    """Lazy through SelectUsersDefender: ``model.from_config("defender", "CatchSyncSelectUsers", attack_num=50)`` keeps the
    configuration, ``.I(dataset=...)`` builds it, ``defense_step()`` returns the flagged user ids.  Afterwards ``scores``,
    ``pair_num``, ``back_num`` (device [U]), ``cell_of`` (device [I]), ``cell_count`` (device [RK_CS_MAX_CELLS]), ``n_cells``,
    ``predLabels`` and ``ranking`` describe the step."""

    victim_name = "CatchSyncSelectUsers"

    def _build(self, score, grid_bits, min_items, attack_num, schedule, form, **config):
        self.score, self.grid_bits, self.min_items, self.attack_num = score, grid_bits, min_items, int(attack_num)
        self.schedule, self.form = schedule, form
        self.scores = self.pair_num = self.back_num = self.cell_of = self.cell_count = self.n_cells = self.predLabels = None
        self._open(config)

    def _check(self):
        check_config(self.score, self.grid_bits, self.min_items, self.schedule, self.form)

    def _detect(self, U, I, rowptr, col, val):
        """The scores of every user on the device, then the flag_count(attack_num, U) users of largest score, ties to the
        lower id."""
        dev = self.device
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
        rnorm = checked_norms("CatchSyncSelectUsers", "rating matrix", U, I, rowptr, col, val)    # nothing further is launched after a refusal
        colptr, crow, cval = transposed(U, I, rowptr, col, val)
        deg_item = torch.empty(I, dtype=torch.int32, device=dev)
        reach = torch.empty(I, dtype=torch.int32, device=dev)
        _lib.check(L.rk_cs_features(U, I, P(rowptr), P(colptr), P(crow), P(deg_item), P(reach), s), "rk_cs_features")
        cell_of = torch.empty(I, dtype=torch.int32, device=dev)
        cell_count = torch.empty(_lib.RK_CS_MAX_CELLS, dtype=torch.int32, device=dev)
        info = torch.empty(4, dtype=torch.int64, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        bad = device_refusal(L.rk_cs_cells(I, P(deg_item), P(reach), int(self.grid_bits), P(cell_of), P(cell_count), P(info), P(status), s),
                             "rk_cs_cells", status)
        if bad:
            raise ValueError(f"CatchSyncSelectUsers: rule {bad[0]} ({_lib.RK_CS_RULES.get(bad[0], '?')}), first at item {bad[1]}")
        M = int(info[0].item())
        order = work_order(rowptr) if self.schedule == "work" else None
        pair_num = torch.empty(U, dtype=torch.int64, device=dev)
        back_num = torch.empty(U, dtype=torch.int64, device=dev)
        _lib.check(L.rk_cs_user_sums(U, P(rowptr), P(col), P(cell_of), P(cell_count), max(M, 1), FORMS.index(self.form), P(order),
                                     P(pair_num), P(back_num), s), "rk_cs_user_sums")
        scores = torch.empty(U, dtype=torch.float32, device=dev)
        _lib.check(L.rk_cs_scores(U, P(rowptr), P(pair_num), P(back_num), P(info), SCORES.index(self.score), int(self.min_items),
                                  P(scores), s), "rk_cs_scores")
        ranked = torch.empty(U, dtype=torch.int32, device=dev)
        _lib.check(L.rk_knn_select(U, P(scores), U, 1, P(ranked), s), "rk_knn_select")
        self.scores, self.pair_num, self.back_num, self.cell_of, self.cell_count = scores, pair_num, back_num, cell_of, cell_count
        self.n_cells = M
        return self._flag(ranked, U)

    @property
    def ranking(self):
        """[(user id, score)] in flag order (descending score, ties to the lower id), built on first use."""
        return self._pairs(self.scores)
