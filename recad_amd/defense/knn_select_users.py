"""KnnSelectUsers: neighbourhood-based fake-user detection on the device.

DegSim (Chirita et al. 2005; Burke / Mobasher et al. 2006): the mean cosine similarity of a profile to its k nearest
neighbours.  It is not in the reference, whose only defender is the spectral PCASelectUsers; include/recad_hip.h states the
exact definition (integer dots, fp32 similarities in a fixed operation order, fp64 mean), csrc/knn.hip computes it without a
U x U matrix, and tests/_knn_restate.py restates it in numpy, bit for bit.

``select="low"`` (the default) flags the ``flag_count(attack_num, U)`` users of SMALLEST DegSim: random-filler profiles
share few items with anybody, and on this project's implicit ml1m-shaped synthetic data 48 of 50 injected profiles are among
the 50 lowest.  ``select="high"`` flags the largest, the side Chirita's explicit-rating / Pearson
setting reports.  Nobody has measured either on real data."""
import torch

from .. import _lib
from .._ratings import checked_norms, transposed
from ._select_users import SelectUsersDefender

SELECTS = ("low", "high")
SCHEDULES = ("work", "natural")


def check_config(k, select, band, schedule):
    """The host-side refusals (ValueError), before any device call."""
    if select not in SELECTS:
        raise ValueError(f"KnnSelectUsers: select = {select!r}, expected one of {SELECTS}")
    if schedule not in SCHEDULES:
        raise ValueError(f"KnnSelectUsers: schedule = {schedule!r}, expected one of {SCHEDULES}")
    if not 1 <= int(k) <= _lib.RK_KNN_MAX_K or int(k) != k:
        raise ValueError(f"KnnSelectUsers: k = {k!r} outside 1..{_lib.RK_KNN_MAX_K}")
    if band is not None and (int(band) != band or band % 64 or not 64 <= band <= _lib.RK_KNN_MAX_BAND):
        raise ValueError(f"KnnSelectUsers: band = {band!r}, expected None or a multiple of 64 in 64..{_lib.RK_KNN_MAX_BAND}")


def work_order(rowptr, col, colptr):
    """Users by descending sum over their items of the item's degree (the LDS adds their workgroup makes), ties to the
    lower id: int32 [U] on the device, torch ops only."""
    U = rowptr.numel() - 1
    deg = (colptr[1:] - colptr[:-1]).to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(U, device=col.device), (rowptr[1:] - rowptr[:-1]).to(torch.int64))
    work = torch.zeros(U, dtype=torch.int64, device=col.device).index_add_(0, rows, deg[col.to(torch.int64)])
    return torch.sort(work, descending=True, stable=True).indices.to(torch.int32).contiguous()


class KnnSelectUsers(SelectUsersDefender):
    """Lazy through SelectUsersDefender: ``model.from_config("defender", "KnnSelectUsers", k=25, attack_num=50)`` keeps the
    configuration, ``.I(dataset=...)`` builds it, ``defense_step()`` returns the flagged user ids.  Afterwards ``scores``
    (device [U]), ``top_similarities`` (device [U, k]), ``predLabels`` and ``ranking`` describe the step."""

    victim_name = "KnnSelectUsers"

    def _build(self, k, attack_num, select, band, schedule, **config):
        self.k, self.attack_num, self.select, self.band, self.schedule = k, int(attack_num), select, band, schedule
        self.scores = self.top_similarities = self.predLabels = None
        self._open(config)

    def _check(self):
        check_config(self.k, self.select, self.band, self.schedule)

    def _detect(self, U, I, rowptr, col, val):
        """DegSim of every user on the device, then the flag_count(attack_num, U) users of smallest (select="low") or largest
        (select="high") DegSim, ties to the lower id."""
        dev, k = self.device, int(self.k)
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
        rnorm = checked_norms("KnnSelectUsers", "rating matrix", U, I, rowptr, col, val)    # nothing further is launched after a refusal
        colptr, crow, cval = transposed(U, I, rowptr, col, val)
        order = work_order(rowptr, col, colptr) if self.schedule == "work" else None
        topw = torch.empty(U, k, dtype=torch.float32, device=dev)
        degsim = torch.empty(U, dtype=torch.float32, device=dev)
        _lib.check(L.rk_knn_degsim(U, I, P(rowptr), P(col), P(val), P(colptr), P(crow), P(cval), P(rnorm), k, int(self.band or 0),
                                   P(order), P(topw), P(degsim), s), "rk_knn_degsim")
        ranked = torch.empty(U, dtype=torch.int32, device=dev)
        _lib.check(L.rk_knn_select(U, P(degsim), U, int(self.select == "high"), P(ranked), s), "rk_knn_select")
        self.scores, self.top_similarities = degsim, topw
        return self._flag(ranked, U)

    @property
    def ranking(self):
        """[(user id, DegSim)] in flag order (ascending for select="low", descending for "high"; ties to the lower id),
        built on first use."""
        return self._pairs(self.scores)
