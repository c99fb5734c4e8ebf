"""What the fit-once victims (ItemKNN, RP3beta, EASE, SLIM) share: a model whose "training" is one deterministic fit of the
dataset's rating matrix.  ``train_step`` fits on first use and does nothing afterwards, the fitted state is module state (a
frozen parameter, buffers, and the ``fitted`` flag), and scoring reads that state and the ratings, which come from the dataset.

A subclass has its ``_build`` (which calls ``_open`` first and creates the state tensors, ``fitted`` among them), ``_check``
(the host-side refusals), ``_fit(dev, rowptr, col, val)`` (the body of the fit) and the two scoring calls ``_score_pairs`` and
``_score_rows``."""
import torch

from .. import _lib
from .._ratings import DeviceRatings
from ..utils import VarDim
from .base import BaseVictim


def matrix_score_pairs(W, n_items, n_users, csr, users, items, n, out, stream):
    """rk_ease_pair_scores on a dense item-item matrix W (EASE's B, SLIM's W: the same orientation)."""
    P = _lib.ptr
    _lib.check(_lib.lib().rk_ease_pair_scores(n_items, n_users, P(W), *map(P, csr), users, items, n, out, stream), "rk_ease_pair_scores")


def matrix_score_rows(W, n_items, csr, user_ids, out, stream):
    """rk_ease_scores on a dense item-item matrix W."""
    P = _lib.ptr
    _lib.check(_lib.lib().rk_ease_scores(n_items, P(W), *map(P, csr), user_ids.numel(), P(user_ids), P(out), stream), "rk_ease_scores")


class FitOnceVictim(BaseVictim):
    label = None                          # "ItemKNN", "EASE", ...: the prefix of every message
    state_noun = None                     # "tables" or "weights": what the CPU refusal says is on the CPU
    _known_fit = None                     # what `fitted` holds, once it has been read back; None: not known

    def _open(self, config):
        self.dataset = config["dataset"]
        self.config = config
        info = self.dataset.info_describe()
        self.num_users, self.num_items = int(info["n_users"]), int(info["n_items"])
        self._ratings = DeviceRatings(self.dataset, self.num_users, self.num_items, self.label)

    def _accepted(self, check=None):
        """False for a configuration that is refused: its state gets 0 rows, and the refusal is raised by the first call that
        would use the state."""
        try:
            (check or self._check)()
            return True
        except (ValueError, TypeError):
            return False

    def _device(self):
        dev = self.fitted.device          # the state moves as one: .to() takes the flag along with the tables
        if dev.type != "cuda":
            raise _lib.HipCallError(f"{self.label} {self.state_noun} are on the CPU: call .to('cuda') first (no CPU fallback)")
        return dev

    def fit(self):
        """Fits the dataset's rating matrix, whether or not the model was fitted before.  A device refusal raises ValueError with
        the rule and where it was broken."""
        self._check()
        dev = self._device()
        _lib.require_gpu()
        self._fit(dev, *self._ratings.on(dev))
        self.fitted.fill_(1)
        self._known_fit = True
        return self

    def _unfit(self):
        """Clears `fitted`.  For a fit that works inside the state's own storage: it calls this first, so that a refusal half
        way leaves the model unfitted."""
        self.fitted.zero_()
        self._known_fit = False

    def _fitted(self):
        """(device, (rowptr, col, val)) of a fitted model: the one read of `fitted`, and the fit when it holds 0."""
        self._check()
        dev = self._device()
        if self._known_fit is None:
            self._known_fit = bool(self.fitted.item())
        if not self._known_fit:
            self.fit()
        return dev, self._ratings.on(dev)

    def _load_from_state_dict(self, *args, **kwargs):
        self._known_fit = None            # `fitted` is about to be overwritten
        return super()._load_from_state_dict(*args, **kwargs)

    def train_step(self, **config):
        """Fits on first use and is a no-op afterwards (workflow.normal_train calls it rec_epoch times).  A fit has no loss:
        the value returned is 0.0."""
        self._fitted()
        return (0.0,)

    # ------------------------------------------------------------------ scoring
    def forward(self, users, items):
        dev, csr = self._fitted()
        users, items = users.long().contiguous(), items.long().contiguous()
        n = users.numel()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        P = _lib.ptr
        self._score_pairs(csr, P(users) if n else None, P(items) if n else None, n, P(out) if n else None, _lib.stream_ptr(dev))
        return out

    def score_matrix(self, user_ids, out):
        """out[len(user_ids), n_items] <- the score of every item for each user (int32 ids on the device), seen items included;
        the batched evaluation then runs rk_topk_rows on it."""
        dev, csr = self._fitted()
        self._score_rows(csr, user_ids, out, _lib.stream_ptr(dev))

    def input_describe(self):
        return {
            "train_step": {},
            "forward": {"users": (torch.int64, (VarDim(comment="batch"))), "items": (torch.int64, (VarDim(comment="batch")))},
        }

    def output_describe(self):
        return {
            "train_step": {"loss": (float, [])},   # always 0.0: a fit has no loss
            "forward": {"unnormalized_scores": (torch.float32, [VarDim(comment="batch")])},
        }
