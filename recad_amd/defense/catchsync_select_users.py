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
from .._ratings import checked_norms, rating_csr, transposed
from ..utils import get_logger
from ..victim.base import BaseVictim
from .pca_select_users import flag_count

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


class CatchSyncSelectUsers(BaseVictim):
    """Lazy like KnnSelectUsers: ``model.from_config("defender", "CatchSyncSelectUsers", attack_num=50)`` keeps the
    configuration, ``.I(dataset=...)`` builds it, ``defense_step()`` returns the flagged user ids.  Afterwards ``scores``,
    ``pair_num``, ``back_num`` (device [U]), ``cell_of`` (device [I]), ``cell_count`` (device [RK_CS_MAX_CELLS]), ``n_cells``,
    ``predLabels`` and ``ranking`` describe the step."""

    victim_name = "CatchSyncSelectUsers"
    scope = "defender"

    def _build(self, score, grid_bits, min_items, attack_num, schedule, form, **config):
        self.dataset = config.get("dataset")
        self.device = torch.device(config.get("device", "cuda"))
        self.score, self.grid_bits, self.min_items, self.attack_num = score, grid_bits, min_items, int(attack_num)
        self.schedule, self.form = schedule, form
        self.logger = get_logger(__name__, level=config.get("logging_level", 20))
        self.scores = self.pair_num = self.back_num = self.cell_of = self.cell_count = self.n_cells = self.predLabels = None
        self._order = self._ranking = None
        self._shape()

    def _shape(self):
        ds = self.dataset
        if ds is None:        # the defence workflow may hand the dataset to defense_step() instead
            self.user_num = self.item_num = None
        elif hasattr(ds, "info_describe") and not isinstance(ds, (tuple, list)):
            info = ds.info_describe()
            self.user_num, self.item_num = int(info["n_users"]), int(info["n_items"])
        elif isinstance(ds, (tuple, list)):
            self.user_num, self.item_num = len(ds[0]) - 1, (int(ds[3]) if len(ds) == 4 else None)
        else:
            self.user_num, self.item_num = int(ds.shape[0]), int(ds.shape[1])

    def forward(self):
        pass

    def train_step(self, **config):
        pass

    def input_describe(self):
        return {"defense_step": {"dataset": (object, [])}}

    def output_describe(self):
        return {"defense_step": {"spam_list": (list, [])}}

    def defense_step(self, **config):
        """The scores of every user on the device, then the flag_count(attack_num, U) users of largest score, ties to the
        lower id.  `dataset=` (optional) replaces the dataset given at .I()."""
        check_config(self.score, self.grid_bits, self.min_items, self.schedule, self.form)
        if config.get("dataset") is not None:
            self.dataset = config["dataset"]
            self._shape()
        if self.dataset is None:
            raise ValueError("CatchSyncSelectUsers.defense_step: no dataset (give one to .I() or to defense_step)")
        _lib.require_gpu()
        dev = self.device
        U, I, rowptr, col, val = rating_csr(self.dataset, dev)
        self.user_num, self.item_num = U, I
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
        rc = L.rk_cs_cells(I, P(deg_item), P(reach), int(self.grid_bits), P(cell_of), P(cell_count), P(info), P(status), s)
        if rc != 0:
            rule, item = status.cpu().tolist()
            if rule:
                raise ValueError(f"CatchSyncSelectUsers: rule {rule} ({_lib.RK_CS_RULES.get(rule, '?')}), first at item {item}")
            _lib.check(rc, "rk_cs_cells")
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
        self.n_cells, self._order = M, ranked
        m = flag_count(self.attack_num, U)
        spam = ranked[:m].cpu().numpy().astype(np.int64)
        self.predLabels = np.zeros(U)
        self.predLabels[spam] = 1
        self._ranking = None
        return spam.tolist()

    @property
    def ranking(self):
        """[(user id, score)] in flag order (descending score, ties to the lower id), built on first use."""
        if self._order is None:
            return None
        if self._ranking is None:
            o = self._order.cpu().numpy()
            d = self.scores.cpu().numpy()[o]
            self._ranking = list(zip(o.tolist(), d.astype(np.float64).tolist()))
        return self._ranking
