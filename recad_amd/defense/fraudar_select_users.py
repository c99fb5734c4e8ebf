"""FraudarSelectUsers: dense-block fake-user detection on the device.

FRAUDAR (Hooi, Song, Beutel, Shah, Shin, Faloutsos, KDD 2016): peel the bipartite rating graph one node at a time, always the
node that carries the least column-weighted edge mass, and keep the densest of the N nested node sets met on the way.  Fake
users who add ratings on popular items cannot lower their own block's score (the paper's camouflage bound), which is what the
filler items of the average, segment and bandwagon attackers are.  include/recad_hip.h states the exact definition (integers
end to end: column weights in 24-bit fixed point, priorities in uint64, the density comparison a 128-bit product),
csrc/fraudar.hip computes it, tests/_fraudar_restate.py restates it on Python integers, word for word.  It is not in the
reference, whose only defender is the spectral PCASelectUsers.

``weight="log"`` (default) is the paper's column weight 1 / ln(deg + log_offset), ``"degree"`` weighs every edge 1 (Charikar's
densest-subgraph peeling).  ``select="block"`` flags the users of the densest block, ascending; ``n_blocks`` > 1 drops a found
block's inner edges and peels again, as the authors' detectMultiple does, and stops at a round without a block.
``select="count"`` flags the ``flag_count(attack_num, U)`` users removed last, for data whose natural core is denser than the
attack.  Not built: rating-weighted edges, flagging items as a workflow step, batch peeling.  More than RK_FD_MAX_NODES = 2^19
users plus items are refused.  DESIGN.md section 22 has the counts on synthetic data and the measured times."""
import math

import numpy as np
import torch

from .. import _lib
from .._ratings import checked_norms, device_refusal, transposed
from ._select_users import SelectUsersDefender, flag_count

WEIGHTS = ("log", "degree")
SELECTS = ("block", "count")
MAX_BLOCKS = 8


def check_config(weight, log_offset, select, n_blocks):
    """The host-side refusals (ValueError), before any device call."""
    if weight not in WEIGHTS:
        raise ValueError(f"FraudarSelectUsers: weight = {weight!r}, expected one of {WEIGHTS}")
    if select not in SELECTS:
        raise ValueError(f"FraudarSelectUsers: select = {select!r}, expected one of {SELECTS}")
    if isinstance(log_offset, bool) or not isinstance(log_offset, (int, float, np.integer, np.floating)) or \
            not math.isfinite(log_offset) or not log_offset > 1:
        raise ValueError(f"FraudarSelectUsers: log_offset = {log_offset!r}, expected a finite number > 1")
    if isinstance(n_blocks, bool) or not isinstance(n_blocks, (int, np.integer)) or not 1 <= n_blocks <= MAX_BLOCKS:
        raise ValueError(f"FraudarSelectUsers: n_blocks = {n_blocks!r}, expected an integer in 1..{MAX_BLOCKS}")
    if n_blocks > 1 and select == "count":
        raise ValueError(f"FraudarSelectUsers: n_blocks = {n_blocks} needs select = 'block' (select = 'count' ranks one peel)")


def weight_table(n_users, weight, log_offset):
    """wtab uint32 [U + 1] on the host, in float64: the weight of a column of d entries in 24-bit fixed point."""
    if weight == "degree":
        return np.full(n_users + 1, _lib.RK_FD_WEIGHT_ONE, dtype=np.uint32)
    d = np.arange(n_users + 1, dtype=np.float64)
    w = np.rint(float(_lib.RK_FD_WEIGHT_ONE) / np.log(d + float(log_offset)))
    return np.minimum(w, float(2 ** 32 - 1)).astype(np.uint32)       # above 2^24 the device refuses it (RK_FD_BAD_WEIGHT)


def without_block(U, rowptr, col, val, in_block):
    """The CSR without the edges whose two ends are in the block (in_block: bool [U + I] on the device)."""
    rows = torch.repeat_interleave(torch.arange(U, device=col.device), (rowptr[1:] - rowptr[:-1]).long())
    keep = ~(in_block[rows] & in_block[U + col.long()])
    new_ptr = torch.zeros(U + 1, dtype=torch.int32, device=col.device)
    new_ptr[1:] = torch.cumsum(torch.bincount(rows[keep], minlength=U), 0).to(torch.int32)
    return new_ptr, col[keep].contiguous(), val[keep].contiguous()


class FraudarSelectUsers(SelectUsersDefender):
    """Lazy through SelectUsersDefender: ``model.from_config("defender", "FraudarSelectUsers", select="count", attack_num=50)``
    keeps the configuration, ``.I(dataset=...)`` builds it, ``defense_step()`` returns the flagged user ids.  Afterwards
    ``step_of``, ``order`` (device int32 [U + I]), ``info`` (device int64 [4]: t*, f, n, f_0) and ``w_item`` (device uint32 words
    in an int32 tensor [I]) describe the first round's peel, ``blocks`` every round's block, ``predLabels`` and ``ranking`` the
    step."""

    victim_name = "FraudarSelectUsers"

    def _build(self, weight, log_offset, select, n_blocks, attack_num, **config):
        self.weight, self.log_offset, self.select, self.n_blocks = weight, log_offset, select, n_blocks
        self.attack_num = int(attack_num)
        self._clear()
        self._open(config)

    def _clear(self):
        self.step_of = self.order = self.info = self.w_item = self.blocks = self.predLabels = None
        self._ranking = None

    def _check(self):
        check_config(self.weight, self.log_offset, self.select, self.n_blocks)

    def _peel(self, U, I, rowptr, col, val):
        """One round on a non-empty CSR: transpose, weights, rk_fd_init, rk_fd_peel -> (step_of, order, info, w_item)."""
        dev = self.device
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
        nnz = int(col.numel())
        colptr, crow, _ = transposed(U, I, rowptr, col, val)
        wtab = torch.from_numpy(weight_table(U, self.weight, self.log_offset).view(np.int32)).to(dev)
        w_item = torch.empty(I, dtype=torch.int32, device=dev)
        pri = torch.empty(U + I, dtype=torch.int64, device=dev)
        info = torch.empty(4, dtype=torch.int64, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        rc = L.rk_fd_init(U, I, nnz, P(rowptr), P(col), P(colptr), P(wtab), P(w_item), P(pri), P(info), P(status), s)
        refused = device_refusal(rc, "rk_fd_init", status)
        if refused:
            rule, index = refused
            raise ValueError(f"FraudarSelectUsers: rule {rule} ({_lib.RK_FD_RULES.get(rule, '?')}), first at index {index} "
                             f"(log_offset = {self.log_offset!r}: a column weight above 1 needs ln(d + log_offset) < 1)")
        order = torch.empty(U + I, dtype=torch.int32, device=dev)
        step_of = torch.empty(U + I, dtype=torch.int32, device=dev)
        _lib.check(L.rk_fd_peel(U, I, nnz, P(rowptr), P(col), P(colptr), P(crow), P(w_item), P(pri), P(order), P(step_of), None, P(info), s),
                   "rk_fd_peel")
        return step_of, order, info, w_item

    def _detect(self, U, I, rowptr, col, val):
        """The peel on the device, then the users of the densest block(s) or the users removed last."""
        if U + I > _lib.RK_FD_MAX_NODES:
            raise ValueError(f"FraudarSelectUsers: {U} users + {I} items, at most RK_FD_MAX_NODES = {_lib.RK_FD_MAX_NODES} nodes")
        self._clear()
        self.blocks = []
        self.predLabels = np.zeros(U)
        if col.numel() == 0:                                  # an empty matrix: no block, nobody flagged
            return []
        checked_norms("FraudarSelectUsers", "rating matrix", U, I, rowptr, col, val)    # nothing further is launched after a refusal
        spam = []
        for r in range(int(self.n_blocks)):
            if col.numel() == 0:
                break
            step_of, order, info, w_item = self._peel(U, I, rowptr, col, val)     # a later round's CSR is a subset of a checked one
            if r == 0:
                self.step_of, self.order, self.info, self.w_item = step_of, order, info, w_item
            t_best, f_best, n_best, _ = info.cpu().tolist()
            if f_best == 0:
                break
            in_block = step_of >= t_best
            members = in_block.nonzero().flatten().cpu().numpy().astype(np.int64)
            users, items = members[members < U], members[members >= U] - U
            self.blocks.append({"users": users, "items": items, "t_best": t_best, "f_best": f_best, "n_best": n_best,
                                "density": f_best / (n_best * float(_lib.RK_FD_WEIGHT_ONE))})
            if self.select == "count":
                o = order.cpu().numpy()[::-1]
                spam = o[o < U][: flag_count(self.attack_num, U)].astype(np.int64).tolist()
                break
            seen = set(spam)
            spam += [u for u in users.tolist() if u not in seen]
            if r + 1 < int(self.n_blocks):
                rowptr, col, val = without_block(U, rowptr, col, val, in_block)
        self.predLabels[np.asarray(spam, dtype=np.int64)] = 1
        return spam

    @property
    def ranking(self):
        """[(user id, step of its removal)] in reverse removal order (the first round's peel), built on first use."""
        if self.order is None:
            return None
        if self._ranking is None:
            o = self.order.cpu().numpy()[::-1]
            o = o[o < self.user_num]
            self._ranking = list(zip(o.tolist(), self.step_of.cpu().numpy()[o].tolist()))
        return self._ranking
