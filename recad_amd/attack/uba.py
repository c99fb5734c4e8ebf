"""UBA attacker on the device (recad/model/attacker/uba.py, registry recad/default.py:210-221).

UBA is AUSH with one change: generate_fake does not draw its template users at random, it asks DSP() (uba.py:169-234) which of
the given target users to copy, and how often.  The GAN (uba.py:236-338, 385-414) is aush.py line for line, so ``UBA`` is a
subclass of ``Aush`` and train_step / input_describe / output_describe are inherited unchanged.  The new ground is the
selection, csrc/uba.hip: for add_num = 1..budget and ten trials each, redraw the target users' ratings (rk_uba_redraw), score
their items over the redrawn matrix with add_num appended copies of each redrawn row (rk_uba_scores) and count how often
selected_ids[0] is among a target user's ten best items; ``prob_mat`` = the hit frequencies, read back once (rk_uba_prob).
``dsp`` below then solves the reference's grouped knapsack on the host (about 50 groups x capacity 100).

Behaviour kept from the reference, quirks included:
  * everything attack/aush.py lists (the generator never trains, ...);
  * ``hops="elementwise"`` (the default): uba.py:99 "cubes" the expanded matrix with ``*``, elementwise, so a target user's
    scores are its own redrawn ratings cubed, the appended copies change nothing, selected_ids[0] (rated 5) is always a
    maximum and can only miss the top ten through the order among tied 5s, which np.argsort leaves unspecified;
  * DSP's weight of column i is i, not i + 1 (a weight 0 exists), its capacity is 100 whatever attack_num is, and its backtrack
    starts at group attack_num (uba.py:182-205): generate_fake returns len(DSP()) rows, not attack_num;
  * where DSP raises (an all-zero prob_mat: AttributeError on an int; no record at the final capacity and value:
    temp_list unbound) or would return an empty list, ``dsp`` raises ValueError and names the case;
  * a chosen user without a rated item outside selected_ids and the targets is an error (np.random.choice on an empty list).
Deviations, both documented in DESIGN.md:
  * the dataset is never written.  The reference redraws train_data_array[target_user_ids[0]] IN PLACE (uba.py:87-91: the row
    is a view until the first vstack), so its dataset keeps the last redraw and a 5 at selected_ids[0];
  * DSP reads ``budget`` columns of prob_mat (1..RK_UBA_MAX_BUDGET) where the reference reads range(6) whatever budget is.
``hops="matrix"`` is this build's opt-in: rows target_user_ids of (E @ E @ E)[:M, M:] with E the expanded (M+N)^2 matrix of
uba.py:95-98, what the name A3_matrix promises.  Among equal scores the build counts a hit when fewer than ten items are
larger or equal-with-a-smaller-id (a stable descending order); ``last_tie_dependent`` counts the cases where the order among
equal scores decides.  The random draws are this build's own (rk_mix64 keyed on seed, add_num, trial, target user, position):
the distribution of random.randint(1, 5), not its numbers.  replay_budget_matrix takes recorded draws instead.
"""
import numpy as np
import torch

from .. import _lib
from ._common import need_dataset, train_csr
from .aush import _FAKE_STREAM, Aush

HOPS = {"elementwise": _lib.RK_UBA_ELEMENTWISE, "matrix": _lib.RK_UBA_MATRIX}
PATHS = {"auto": _lib.RK_UBA_PATH_AUTO, "lds": _lib.RK_UBA_PATH_LDS, "work": _lib.RK_UBA_PATH_WORK}
CAPACITY = 100      # uba.py:194


def dsp(prob_mat, target_user_ids, attack_num):
    """DSP() after budget_matrix() (uba.py:173-234) with DSP_part (uba.py:142-166): the grouped knapsack over prob_mat
    [n_targets, budget] -- one group per target user with a nonzero entry, item k of a group = a nonzero column i with
    weight i and value prob_mat[t, i] -- of capacity 100, every improvement recorded, then the reference's walk back through
    the records from group ``attack_num``.  Returns the chosen users, each repeated by its weight.  Values stay np.float64
    so that round() is numpy's, as in the reference.  ValueError where the reference raises or returns nothing."""
    x = np.asarray(prob_mat, dtype=np.float64)
    users = list(target_user_ids)
    if x.ndim != 2 or x.shape[0] != len(users):
        raise ValueError(f"dsp: prob_mat {x.shape} does not have one row per target user ({len(users)})")
    groups = []                                             # (user, weights, values) of the non-empty groups, uba.py:179-190
    for t, user in enumerate(users):
        cols = [i for i in range(x.shape[1]) if x[t, i] != 0]
        if cols:
            groups.append((user, cols, [x[t, i] for i in cols]))
    if not groups:
        raise ValueError("dsp: prob_mat is all zero: no target user ever has the selected item in its top ten "
                         "(the reference fails here with an AttributeError)")
    best = [0] * (CAPACITY + 1)
    records = []                                            # (group from 1, item, capacity, rounded best value) in order
    for g, (_, weights, values) in enumerate(groups, start=1):
        for cap in range(CAPACITY, 0, -1):
            for k, (wk, vk) in enumerate(zip(weights, values)):
                if cap - wk < 0:
                    continue
                best[cap] = max(best[cap], best[cap - wk] + vk)
                if best[cap - wk] + vk >= best[cap]:        # read again after the update: with weight 0 it always holds
                    records.append((g, k, cap, round(best[cap], 2)))
    top = round(best[CAPACITY], 1)
    last = None
    for r in records:
        if r[2] == CAPACITY and r[3] == top:
            last = r
    if last is None:
        raise ValueError(f"dsp: no knapsack record reaches capacity {CAPACITY} with the value {top} "
                         "(the reference fails here with an unbound temp_list)")
    known = set(records)
    group, item, cap, value = attack_num, last[1], CAPACITY, top
    chosen = {}
    while (group, item, cap, value) in known:
        user, weights, values = groups[group - 1]
        chosen[user] = weights[item]
        cap = round(cap - weights[item], 2)
        value = round(value - values[item], 2)
        for r in records:                                   # the first record of another group at what is left
            if r[2] == cap and r[3] == value and r[0] != group:
                group, item = r[0], r[1]
                break
    out = [user for user, weight in chosen.items() for _ in range(weight)]
    if not out:
        raise ValueError(f"dsp: the walk back from group attack_num = {attack_num} ({len(groups)} non-empty groups) chose no user "
                         "(the reference returns an empty list here and fails in sample_fillers)")
    return out


def check_settings(n_users, n_items, selected_ids, target_user_ids, budget, hops, path="auto"):
    """The refusals of UBA's own settings, host only: (target users as int32 array, budget, mode, path)."""
    if hops not in HOPS:
        raise ValueError(f"UBA: hops must be one of {sorted(HOPS)}, not {hops!r}")
    if path not in PATHS:
        raise ValueError(f"UBA: path must be one of {sorted(PATHS)}, not {path!r}")
    if int(budget) != budget or not 1 <= int(budget) <= _lib.RK_UBA_MAX_BUDGET:
        raise ValueError(f"UBA: budget must be an integer in [1, {_lib.RK_UBA_MAX_BUDGET}], not {budget!r}")
    tu = [int(u) for u in target_user_ids]
    if not 1 <= len(tu) <= _lib.RK_UBA_MAX_TARGETS:
        raise ValueError(f"UBA: target_user_ids must hold 1..{_lib.RK_UBA_MAX_TARGETS} users, not {len(tu)}")
    if min(tu) < 0 or max(tu) >= n_users:
        raise ValueError(f"UBA: target_user_ids must lie in [0, {n_users})")
    if len(set(tu)) != len(tu):
        raise ValueError("UBA: target_user_ids lists a user twice")
    if len(selected_ids) == 0 or not 0 <= int(selected_ids[0]) < n_items:
        raise ValueError(f"UBA: selected_ids[0] must be an item id in [0, {n_items})")
    if path == "lds" and n_users > _lib.RK_UBA_LDS_USERS:
        raise ValueError(f"UBA: the LDS path holds at most {_lib.RK_UBA_LDS_USERS} users, the data has {n_users}")
    if hops == "matrix" and (n_users + len(tu) * int(budget)) * 125.0 * n_items > 2.0 ** 53:
        raise ValueError(f"UBA: three-hop scores over {n_users} users x {n_items} items can exceed 2^53")
    return np.asarray(tu, dtype=np.int32), int(budget), HOPS[hops], PATHS[path]


def rating_csc(n_users, n_items, ptr, idx, val):
    """(colptr, row, val) of the transpose of a rating CSR, rows ascending inside a column."""
    ptr, idx, val = np.asarray(ptr), np.asarray(idx), np.asarray(val)
    rows = np.repeat(np.arange(n_users, dtype=np.int32), np.diff(ptr))
    order = np.argsort(idx, kind="stable")
    colptr = np.zeros(n_items + 1, dtype=np.int64)
    colptr[1:] = np.cumsum(np.bincount(idx, minlength=n_items))
    return colptr.astype(np.int32), rows[order], val[order].astype(np.float32)


def side_layout(ptr, idx, target_users, s):
    """side_ptr [n_targets + 1] of the redrawn rows: a target user's rated items, plus s when it is not among them."""
    ptr, idx = np.asarray(ptr), np.asarray(idx)
    lens = [int(ptr[u + 1] - ptr[u]) + (0 if s in idx[ptr[u]:ptr[u + 1]] else 1) for u in target_users]
    out = np.zeros(len(lens) + 1, dtype=np.int32)
    out[1:] = np.cumsum(lens)
    return out


class UBA(Aush):
    """``model.from_config("attacker", "uba", **kw)``; ``.I(dataset=explicit)`` builds it.  train_step is Aush's.
    ``budget_matrix()`` -> prob_mat [n_targets, budget]; ``DSP()`` -> the template users; ``generate_fake(target_id_list=...)``
    -> len(DSP()) x n_items float32."""

    victim_name = "uba"
    scope = "attacker"
    user_args = "dataset, path"      # path: "auto" | "lds" | "work", where rk_uba_scores keeps its weight vectors

    def _build(self, target_user_ids, budget, hops, seed, selected_ids, **config):
        ds = need_dataset(self, config)
        U, I, ptr, idx, val = train_csr(ds)
        path = config.pop("path", "auto")
        tu, budget, mode, path = check_settings(U, I, list(selected_ids), target_user_ids, budget, hops, path)
        seed = int(np.random.randint(0, 2 ** 31 - 1) if seed is None else seed)
        super()._build(selected_ids=selected_ids, seed=seed, **config)
        self.target_user_id = [int(u) for u in tu]
        self.budget, self.hops = budget, hops
        self._mode, self._path, self._tu = mode, path, tu
        self._s = int(list(selected_ids)[0])
        self.side_ptr = side_layout(ptr, idx, tu, self._s)
        self._side_cap = int(self.side_ptr[-1])
        colptr, crow, cval = rating_csc(U, I, ptr, idx, val)
        dev = self.device
        self._colptr, self._crow, self._cval = (torch.as_tensor(a).to(dev) for a in (colptr, crow, cval))
        nb = _lib.C.c_int64()
        _lib.check(_lib.lib().rk_uba_workspace_bytes(U, I, len(tu), self._side_cap, budget, _lib.C.byref(nb)), "rk_uba_workspace_bytes")
        self.scratch_bytes = int(nb.value)
        self._budget_calls = 0
        self.last_tie_dependent = None
        self.last_templates = None

    # ------------------------------------------------------------------ uba.py:81-140
    def _prob(self, draws, call):
        n = len(self._tu)
        prob = np.zeros((n, self.budget), dtype=np.float64)
        ties = _lib.C.c_int32()
        P = _lib.ptr
        _lib.check(_lib.lib().rk_uba_prob(self.n_users, self.n_items, self._col.numel(), P(self._rowptr), P(self._col), P(self._colptr),
                                          P(self._crow), P(self._cval), self._tu.ctypes.data_as(_lib.C.c_void_p), n, self._s, self.budget,
                                          self._mode, self._path, P(draws), (self.seed + 0x9E3779B9 * call) & (2 ** 64 - 1), self._side_cap,
                                          prob.ctypes.data_as(_lib.C.c_void_p), _lib.C.byref(ties), _lib.stream_ptr(self.device)), "rk_uba_prob")
        self.last_tie_dependent = int(ties.value)
        return prob

    def budget_matrix(self):
        """prob_mat [n_targets, budget]: entry (t, b - 1) = in how many of ten redraws with add_num = b the selected item is in
        target user t's top ten, / 10.  Each call draws a fresh stream.  last_tie_dependent = the cases decided by the order
        among equal scores."""
        call = self._budget_calls
        self._budget_calls += 1
        return self._prob(None, call)

    def replay_budget_matrix(self, draws):
        """budget_matrix on recorded draws [budget, 10, side_ptr[-1]]: slab (b - 1, trial) holds the redrawn ratings of the
        target users' rows in side_ptr's layout (rated items ascending with s in its place; the entry at s is ignored)."""
        d = np.ascontiguousarray(np.asarray(draws).reshape(self.budget, _lib.RK_UBA_TRIALS, self._side_cap), dtype=np.int32)
        if d.size and (d.min() < 1 or d.max() > 5):
            raise ValueError("UBA: replayed draws must lie in 1..5")
        return self._prob(torch.as_tensor(d).to(self.device), 0)

    def DSP(self):
        return dsp(self.budget_matrix(), self.target_user_id, self.attack_num)

    # ------------------------------------------------------------------ uba.py:340-379
    def generate_fake(self, **kwargs):
        """len(DSP()) rows on the DSP() users as templates: fillers drawn from each one's own ratings, 5 at every target, the
        generator's values at selected_ids rounded half to even and clipped to [1, 5] (Aush's _sample and _fake)."""
        pool = self._pool(kwargs["target_id_list"])
        chosen = np.asarray(self.DSP(), dtype=np.int32)
        sizes = np.diff(pool["ptr"].cpu().numpy())[chosen]
        if (sizes == 0).any():
            raise ValueError(f"UBA.generate_fake: template user {int(chosen[sizes == 0][0])} has no rated item outside selected_ids and "
                             "the targets")
        call = self._fake_calls
        self._fake_calls += 1
        users = torch.as_tensor(chosen).to(self.device)
        rows = self._rows(len(chosen))
        self._sample(users, rows, pool=pool, stream_id=_FAKE_STREAM | call)
        self.last_templates = chosen
        return self._fake(users, rows, pool, len(chosen))
