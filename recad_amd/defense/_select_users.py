"""What the select-users defenders (PCA, KNN, CatchSync, Fraudar) share: a lazy object that keeps its configuration, takes its
dataset at ``.I()`` or at the step, and whose ``defense_step()`` turns the dataset's rating matrix into a list of flagged user
ids on the device.

A subclass has its ``_build`` (which stores its own keys, sets its result attributes to None and calls ``_open`` last),
``_check`` (the host-side refusals; none by default) and ``_detect(U, I, rowptr, col, val)`` (the body of the step, which returns
the flagged ids).  A detector that ranks every user ends ``_detect`` with ``_flag`` and serves its ranking from ``_pairs``."""
import math

import numpy as np
import torch

from .. import _lib
from .._ratings import rating_csr
from ..utils import get_logger
from ..victim.base import BaseVictim


def flag_count(attack_num, n_users):
    """Number of users the reference flags: #{i >= 0 : i < (attack_num / U) * U} in float64 (PCASelectUsers.py:34,85),
    which rounding can make attack_num + 1.  Capped at U."""
    bound = (attack_num / n_users) * n_users
    return min(int(n_users), max(0, math.ceil(bound)))


class SelectUsersDefender(BaseVictim):
    scope = "defender"

    def _open(self, config):
        self.dataset = config.get("dataset")
        self.device = torch.device(config.get("device", "cuda"))
        self.logger = get_logger(type(self).__module__, level=config.get("logging_level", 20))
        self._order = self._pair_list = None
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

    def _check(self):
        pass

    def defense_step(self, **config):
        """The flagged user ids.  `dataset=` (optional) replaces the dataset given at .I() -- the workflow hands over the
        poisoned one it is meant to clean.  The host-side refusals come first, then the missing dataset, and only then the device."""
        self._check()
        if config.get("dataset") is not None:
            self.dataset = config["dataset"]
            self._shape()
        if self.dataset is None:
            raise ValueError(f"{type(self).__name__}.defense_step: no dataset (give one to .I() or to defense_step)")
        _lib.require_gpu()
        U, I, rowptr, col, val = rating_csr(self.dataset, self.device)
        self.user_num, self.item_num = U, I
        return self._detect(U, I, rowptr, col, val)

    def _flag(self, order, U):
        """The first flag_count(attack_num, U) ids of `order` (int32 [U], every user in flag order) as a list; fills predLabels
        and keeps the order for _pairs."""
        spam = order[:flag_count(self.attack_num, U)].cpu().numpy().astype(np.int64)
        self.predLabels = np.zeros(U)
        self.predLabels[spam] = 1
        self._order, self._pair_list = order, None
        return spam.tolist()

    def _pairs(self, values):
        """[(user id, float64 value)] in the order _flag was given, built on first use; None before the first step."""
        if self._order is None:
            return None
        if self._pair_list is None:
            o = self._order.cpu().numpy()
            self._pair_list = list(zip(o.tolist(), values.cpu().numpy()[o].astype(np.float64).tolist()))
        return self._pair_list
