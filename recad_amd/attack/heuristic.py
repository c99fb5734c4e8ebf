"""The heuristic attackers on the device: average, segment and bandwagon (recad/model/attacker/heuristic.py:85-325, registry
recad/default.py:136-158).  ``random`` stays workflow.RandomAttack on the host (attack/aush.py, RandomAttacker).

csrc/heuristic.hip does the work: the per-item counts and means and the global mean / population std of the train ratings in
two passes over the rating CSR (the reference masks all ratings once per distinct item, heuristic.py:94-98), the popularity
ranking, and the attack_num x n_items profiles built in device memory.  The statistics are read back once, at .I().

Behaviour kept from the reference, quirks included:
  * with rate = attack_num // len(target_id_list), row r < rate * len(target_id_list) rates target r // rate with 5; the
    remaining attack_num - rate * len(target_id_list) rows rate NO target, and with more targets than rows (rate 0) no row
    does (the slices of heuristic.py:118-121);
  * the average attack draws a rated item's filler value from N(item mean, item mean): item_std_dict holds the mean
    (heuristic.py:98).  An item nobody rated gets N(global mean, global std);
  * segment fillers are 1, bandwagon fillers N(global mean, global std); normal values are rounded half to even, then
    clipped to [1, 5].
Differences, on purpose:
  * the reference's BandwagonAttack.from_config reads the ``segment`` defaults (heuristic.py:264-266), so its registry entry
    never reaches it; this build uses the ``bandwagon`` entry (selected_ids [], hence the 11 most rated items);
  * among equally rated items the popularity rule takes the larger id first (the reference's order there is an unstable
    sort's); items nobody rated are never selected;
  * the statistics are those of the rating CSR, where a (user, item) pair stored twice is one rating, the sum (as in
    train_mat); the reference's train_kvr rows count it twice;
  * the random draws are this build's own (rk_mix64 keyed on seed, call, row and draw): the same distributions as the
    reference's np.random calls, not the same numbers.  replay_fake takes the reference's draws instead.
"""
import numpy as np
import torch

from .. import _lib
from ..utils import VarDim
from ..victim.base import BaseVictim
from ._common import open_build

_FAKE_STREAM = 1 << 62
POPULAR_K = 11      # heuristic.py:259


class _Heuristic(BaseVictim):
    """``model.from_config("attacker", name, **kw)`` keeps the configuration, ``.I(dataset=explicit)`` computes the rating
    statistics on the device, ``generate_fake(target_id_list=...)`` returns an attack_num x n_items float32 array.  There is
    no train_step: both workflows skip the attacker's training."""

    scope = "attacker"
    mode = None                 # RK_HEUR_* filler value rule
    has_selected = False
    popular_when_empty = False

    def _build(self, attack_num, filler_num, seed, selected_ids=(), **config):
        _, U, I, ptr, idx, val = open_build(self, config)
        self.attack_num, self.filler_num = int(attack_num), int(filler_num)
        self.seed = int(np.random.randint(0, 2 ** 31 - 1) if seed is None else seed)
        self.n_users, self.n_items = U, I
        if self.attack_num <= 0:
            raise ValueError("attack_num must be positive")
        if not 0 < self.filler_num <= _lib.RK_HEUR_MAX_FILLER:
            raise ValueError(f"filler_num must be in [1, {_lib.RK_HEUR_MAX_FILLER}]")
        dev, L, P = self.device, _lib.lib(), _lib.ptr
        col = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
        rating = torch.as_tensor(np.ascontiguousarray(val, dtype=np.float32)).to(dev)
        self._item_count = torch.empty(I, dtype=torch.int32, device=dev)
        self._item_mean = torch.empty(I, dtype=torch.float64, device=dev)
        glob = torch.empty(2, dtype=torch.float64, device=dev)
        n_rated = torch.empty(1, dtype=torch.int32, device=dev)
        nnz = int(col.numel())
        _lib.check(L.rk_heur_item_stats(I, nnz, P(col) if nnz else None, P(rating) if nnz else None, P(self._item_count),
                                        P(self._item_mean), P(glob), P(n_rated), _lib.stream_ptr(dev)), "rk_heur_item_stats")
        self.item_count = self._item_count.cpu().numpy()
        self.item_mean = self._item_mean.cpu().numpy()
        self.global_mean, self.global_std = (float(x) for x in glob.cpu().numpy())
        self.n_rated = int(n_rated.cpu().numpy()[0])
        sel = [int(s) for s in selected_ids] if self.has_selected else []
        if self.popular_when_empty and not sel:
            sel = self.popular(POPULAR_K)[0]
        self.selected_ids = sel
        self._check_ids(sel, "selected_ids", _lib.RK_HEUR_MAX_SELECT)
        self._fake_calls = 0

    def popular(self, k):
        """(ids, counts) of the k most rated items, most rated first, the larger id first among equal counts; fewer than k
        when fewer items are rated."""
        dev, P = self.device, _lib.ptr
        ids = torch.empty(k, dtype=torch.int32, device=dev)
        counts = torch.empty(k, dtype=torch.int32, device=dev)
        n = _lib.C.c_int32()
        _lib.check(_lib.lib().rk_heur_popular(self.n_items, P(self._item_count), k, P(ids), P(counts), _lib.C.byref(n),
                                              _lib.stream_ptr(dev)), "rk_heur_popular")
        return ids.cpu().numpy()[: n.value].tolist(), counts.cpu().numpy()[: n.value].tolist()

    def _check_ids(self, ids, what, limit):
        if len(ids) > limit:
            raise ValueError(f"{what}: at most {limit} ids")
        if ids and (min(ids) < 0 or max(ids) >= self.n_items):
            raise ValueError(f"{what} must lie in [0, {self.n_items})")

    def _targets(self, target_id_list):
        tg = [int(t) for t in target_id_list]
        if not tg:
            raise ValueError("target_id_list is empty")
        self._check_ids(tg, "target_id_list", _lib.RK_HEUR_MAX_TARGETS)
        pool = self.n_items - len(set(tg) | set(self.selected_ids))
        if self.filler_num > pool:
            raise ValueError(f"filler_num {self.filler_num} is above the {pool} items outside the targets and selected ids")
        return tg

    def _generate(self, tg, rows, stream, cols=None, vals=None):
        out = torch.empty(rows, self.n_items, dtype=torch.float32, device=self.device)
        P, I32 = _lib.ptr, _lib.C.c_int32
        sel = self.selected_ids
        _lib.check(_lib.lib().rk_heur_generate(rows, self.n_items, self.filler_num, (I32 * len(tg))(*tg), len(tg),
                                               (I32 * len(sel))(*sel) if sel else None, len(sel), self.mode, self.global_mean,
                                               self.global_std, P(self._item_mean), P(self._item_count), P(cols), P(vals), self.seed,
                                               stream, P(out), _lib.stream_ptr(self.device)), "rk_heur_generate")
        return out.cpu().numpy()

    # ------------------------------------------------------------------ description (heuristic.py:153-165)
    def forward(self):
        pass

    def input_describe(self):
        return {"generate_fake": {"target_id_list": (list, VarDim())}}

    def output_describe(self):
        return {"generate_fake": {"fake_profile": (np.ndarray, (self.attack_num, self.n_items))}}

    # ------------------------------------------------------------------ heuristic.py:115-151, 191-220, 274-311
    def generate_fake(self, **kwargs):
        """attack_num rows; every call draws from a fresh stream of the device RNG."""
        tg = self._targets(kwargs["target_id_list"])
        call = self._fake_calls
        self._fake_calls += 1
        return self._generate(tg, self.attack_num, _FAKE_STREAM | call)

    def replay_fake(self, cols, vals, target_id_list):
        """generate_fake on given draws: cols [n, filler_num] item ids (distinct in a row, outside the targets and selected
        ids), vals [n, filler_num] the float64 values before rounding (None for the segment attack, whose fillers are 1)."""
        tg = self._targets(target_id_list)
        cols = np.asarray(cols)
        if cols.ndim != 2 or cols.shape[1] != self.filler_num or cols.shape[0] == 0:
            raise ValueError(f"replay_fake: cols must be [n, {self.filler_num}]")
        if cols.min() < 0 or cols.max() >= self.n_items:
            raise ValueError(f"replay_fake: cols must lie in [0, {self.n_items})")
        srt = np.sort(cols, axis=1)
        if (srt[:, 1:] == srt[:, :-1]).any() or np.isin(cols, list(set(tg) | set(self.selected_ids))).any():
            raise ValueError("replay_fake: a row's cols must be distinct and outside the targets and selected ids")
        c = torch.as_tensor(np.ascontiguousarray(cols, dtype=np.int32)).to(self.device)
        v = None
        if self.mode != _lib.RK_HEUR_ONES:
            vals = np.asarray(vals, dtype=np.float64)
            if vals.shape != cols.shape:
                raise ValueError("replay_fake: vals must have the shape of cols")
            v = torch.as_tensor(np.ascontiguousarray(vals)).to(self.device)
        return self._generate(tg, cols.shape[0], 0, c, v)


class AverageAttack(_Heuristic):
    """heuristic.py:85-165: fillers valued N(item mean, item mean) (the reference's quirk), no selected items."""

    victim_name = "average"
    mode = _lib.RK_HEUR_ITEM


class SegmentAttack(_Heuristic):
    """heuristic.py:168-234: the selected items rated 5 on every row, fillers 1."""

    victim_name = "segment"
    mode = _lib.RK_HEUR_ONES
    has_selected = True


class BandwagonAttack(_Heuristic):
    """heuristic.py:237-325: the selected items rated 5 on every row, fillers N(global mean, global std).  An empty
    selected_ids (this build's default: the registry's ``bandwagon`` entry, which the reference's from_config never reads)
    becomes the 11 most rated items, larger id first among equal counts."""

    victim_name = "bandwagon"
    mode = _lib.RK_HEUR_GLOBAL
    has_selected = True
    popular_when_empty = True
