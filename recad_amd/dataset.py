"""Implicit-feedback dataset feeding the victim hot path.

This is the build's own thin counterpart of recad/dataset/implicit.py: it
exposes the same object contract the victims and the workflow consume --
``info_describe()`` (n_users, n_items, train/valid/test dicts, graph), ``generate_batch()``
(dicts of int64 device tensors, last batch short), ``inject_data``, ``reset``,
``partial_sample`` -- but keeps interactions as CSR arrays, samples with vectorised numpy
instead of per-draw Python loops, and builds the normalised adjacency on the GPU
(rk_build_norm_adj) instead of scipy dok/lil.
"""
import random
from copy import copy

import numpy as np
import torch

from .default import DATASET_EXPLICIT, DATASET_IMPLICIT
from .utils import VarDim, get_logger


def _dict_to_csr(d, n_rows=None):
    users = np.fromiter((int(u) for u in d.keys()), dtype=np.int64, count=len(d))
    n = int(users.max()) + 1 if len(users) else 0
    n_rows = max(n, n_rows or 0)
    cnt = np.zeros(n_rows, dtype=np.int64)
    for u, items in d.items():
        cnt[int(u)] = len(items)
    ptr = np.zeros(n_rows + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(cnt)
    idx = np.zeros(ptr[-1], dtype=np.int32)
    for u, items in d.items():
        if len(items):
            idx[ptr[int(u)]:ptr[int(u) + 1]] = np.asarray(items, dtype=np.int32)
    return ptr, idx


def _csr_to_dict(ptr, idx):
    return {int(u): idx[ptr[u]:ptr[u + 1]].tolist() for u in range(len(ptr) - 1) if ptr[u + 1] > ptr[u]}


def _pad_csr(csr, n_rows):
    ptr, idx = csr
    if len(ptr) - 1 >= n_rows:
        return np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int32)
    out = np.full(n_rows + 1, ptr[-1], dtype=np.int64)
    out[: len(ptr)] = ptr
    return out, np.asarray(idx, dtype=np.int32)


def _sorted_unique_rows(ptr, idx):
    """Sort item ids within each user and drop duplicates (the scipy CSR the reference builds
    at implicit.py:206-209 sums duplicates; interactions are unique per user anyway)."""
    n = len(ptr) - 1
    users = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    width = int(idx.max()) + 1 if len(idx) else 1
    keys = users * width + idx.astype(np.int64)
    if len(keys) > 1 and not bool(np.all(keys[1:] > keys[:-1])):   # (lists that are already sorted and unique skip the sort: 0.6 vs 10.6 ms at ml1m size)
        keys = np.unique(keys)
    cnt = np.bincount(keys // width, minlength=n)
    out = np.zeros(n + 1, dtype=np.int64)
    out[1:] = np.cumsum(cnt)
    return out, (keys % width).astype(np.int32)


def csv_to_dict(path, rating_filter=4):
    """recad/dataset/implicit.py:94-104: keep rating >= filter, time order, first occurrence."""
    import pandas as pd

    df = pd.read_csv(path).sort_values("timestamp")
    df = df[df["rating"] >= rating_filter]
    out = {}
    for u, i in zip(df["user_id"].to_numpy(), df["item_id"].to_numpy()):
        lst = out.setdefault(int(u), [])
        if int(i) not in lst:
            lst.append(int(i))
    return out


class ImplicitData:
    def __init__(self, **config):
        self.config = config
        self.logger = get_logger(f"{__name__}:{self.dataset_name}", level=config["logging_level"])
        self._mode = "train"
        self._dicts = {}
        splits = {}
        for split in ("train", "valid", "test"):
            if config.get(f"{split}_csr") is not None:
                splits[split] = tuple(np.asarray(a) for a in config[f"{split}_csr"])
            elif config.get(f"{split}_dict") is not None:
                self._dicts[split] = config[f"{split}_dict"]
                splits[split] = _dict_to_csr(config[f"{split}_dict"])
            elif config.get(f"path_{split}"):
                self._dicts[split] = csv_to_dict(config[f"path_{split}"], config["rating_filter"])
                splits[split] = _dict_to_csr(self._dicts[split])
            else:
                splits[split] = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))
        # n_users / n_items = max id + 1 over train, valid, test (implicit.py:229-230,194-195)
        self.n_users = max(len(p) - 1 for p, _ in splits.values())
        # users with empty lists at the tail do not count in the reference (only non-empty rows do)
        self.n_users = max((int(np.nonzero(np.diff(p))[0].max()) + 1 if len(i) else 0) for p, i in splits.values())
        self.n_items = max((int(i.max()) + 1 if len(i) else 0) for _, i in splits.values())
        self._csr = {k: _pad_csr(v, self.n_users) for k, v in splits.items()}
        self._csr = {k: (p[: self.n_users + 1], i[: p[self.n_users]]) for k, (p, i) in self._csr.items()}
        self.traindataSize = int(self._csr["train"][0][-1])
        self.validDataSize = int(self._csr["valid"][0][-1])
        self.testDataSize = int(self._csr["test"][0][-1])
        # The reference builds UserItemNet (hence the graph AND the BPR positives) from whichever
        # split read_data() saw last, i.e. the TEST edges (implicit.py:173-192,206-209,233-235).
        src = "test" if config["graph_source"] == "reference" else "train"
        self._net = _sorted_unique_rows(*self._csr[src])
        self._net_keys = (np.repeat(np.arange(self.n_users, dtype=np.int64), np.diff(self._net[0])) * self.n_items
                          + self._net[1].astype(np.int64))
        self._train_sorted = None
        self._heldout_sorted = {}
        self._graph = None
        self._graph_coo = None
        seed = config.get("seed", None)
        self._rng = np.random.default_rng(np.random.randint(0, 2 ** 31 - 1) if seed is None else seed)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_config(cls, name, **user_config):
        config = {k: copy(v) for k, v in DATASET_IMPLICIT.items()}
        for k in ("train_csr", "valid_csr", "test_csr", "seed"):
            config[k] = None
        for k, v in user_config.items():
            if k == "download":
                continue
            if k not in config:
                get_logger(__name__).debug(f"Unexpected key [{k}] for {cls}")
            config[k] = v
        inst = object.__new__(cls)
        inst._dataset_name = name
        inst._init_config = config
        inst.__init__(**config)
        return inst

    @property
    def dataset_name(self):
        return getattr(self, "_dataset_name", type(self).__name__)

    def reset(self, **kwargs):
        config = copy(self._init_config)
        for k, v in kwargs.items():
            if k not in config:
                raise ValueError(f"reset arg {k} should be in {list(config)}")
            config[k] = v
            if k.endswith("_dict") and v is not None:
                config[k.replace("_dict", "_csr")] = None
            if k.endswith("_csr") and v is not None:
                config[k.replace("_csr", "_dict")] = None
        # splits not overridden carry over as CSR (cheap, no dict rebuild)
        for split in ("train", "valid", "test"):
            if config.get(f"{split}_csr") is None and config.get(f"{split}_dict") is None:
                config[f"{split}_csr"] = self._csr[split]
        return type(self).from_config(self.dataset_name, **config)

    # ------------------------------------------------------------------ description
    def _dict(self, split):
        if split not in self._dicts:
            self._dicts[split] = _csr_to_dict(*self._csr[split])
        return self._dicts[split]

    @property
    def train_dict(self):
        return self._dict("train")

    @property
    def valid_dict(self):
        return self._dict("valid")

    @property
    def test_dict(self):
        return self._dict("test")

    def train_csr_sorted(self):
        """user -> sorted unique train items (seen-item lists for evaluation)."""
        if self._train_sorted is None:
            self._train_sorted = _sorted_unique_rows(*self._csr["train"])
        return self._train_sorted

    def heldout_csr(self, split, device=None):
        """user -> sorted unique items of the "valid" / "test" split: the ground truth of evaluate.heldout_quality.  Host arrays, or
        with `device` their int32 copies there; both are made once per split (and device)."""
        if split not in ("valid", "test"):
            raise ValueError(f"heldout_csr: split must be 'valid' or 'test', got {split!r}")
        if split not in self._heldout_sorted:
            self._heldout_sorted[split] = _sorted_unique_rows(*self._csr[split])
        if device is None:
            return self._heldout_sorted[split]
        key = (split, torch.device(device))
        if key not in self._heldout_sorted:
            self._heldout_sorted[key] = tuple(torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device=key[1])
                                              for a in self._heldout_sorted[split])
        return self._heldout_sorted[key]

    @property
    def allPos(self):
        ptr, idx = self._net
        return [idx[ptr[u]:ptr[u + 1]] for u in range(self.n_users)]

    def graph_csr(self):
        """Normalised adjacency as a device CSR (built once, on the GPU)."""
        if self._graph is None:
            from .graph import CsrGraph
            self._graph = CsrGraph.from_user_item_csr(self.n_users, self.n_items, self._net[0], self._net[1],
                                                      self.config["device"])
        return self._graph

    def getSparseGraph(self):
        """The graph in the reference's format (coalesced torch sparse COO, implicit.py:243-298)."""
        if self._graph_coo is None:
            self._graph_coo = self.graph_csr().to_torch_coo()
        return self._graph_coo

    def batch_describe(self):
        if self._mode == "train" and self.config["sample"] == "pairwise":
            b = VarDim(max=self.config["pairwise_batch_size"], comment="batch")
            return {"users": (torch.int64, b), "positive_items": (torch.int64, b), "negative_items": (torch.int64, b)}
        if self._mode == "train" and self.config["sample"] == "pointwise":
            b = VarDim(max=self.config["pointwise_batch_size"], comment="batch")
            return {"users": (torch.int64, b), "items": (torch.int64, b), "labels": (torch.int64, b)}
        b = VarDim(max=self.config["test_batch_size"], comment="batch")
        return {"users": (torch.int64, b), "positive_items": (list, b), "ground_truth": (list, b)}

    class _Info(dict):
        """info_describe() result; the dict/graph views are materialised on first access."""

        def __init__(self, ds, base):
            super().__init__(base)
            self._ds = ds

        def __missing__(self, key):
            ds = self._ds
            lazy = {"train_dict": lambda: ds.train_dict, "valid_dict": lambda: ds.valid_dict,
                    "test_dict": lambda: ds.test_dict}
            if ds.config["need_graph"]:
                lazy["graph"] = ds.getSparseGraph
                lazy["graph_csr"] = ds.graph_csr
            if key not in lazy:
                raise KeyError(key)
            self[key] = lazy[key]()
            return self[key]

        def get(self, key, default=None):
            try:
                return self[key]
            except KeyError:
                return default

    def info_describe(self):
        return ImplicitData._Info(self, {
            "n_users": self.n_users, "n_items": self.n_items, "train_interactions": self.traindataSize,
            "valid_interactions": self.validDataSize, "test_interactions": self.testDataSize,
            "batch_describe": self.batch_describe(),
        })

    def mode(self):
        return self._mode

    def switch_mode(self, mode):
        assert mode in ["train", "test", "validate"]
        self._mode = mode

    # ------------------------------------------------------------------ samplers
    def pairwise_sample(self):
        """BPR triplets with the semantics of recad/dataset/implicit.py:50-74: traindataSize
        uniform user draws (with replacement), users without positives skipped, uniform
        positive, negative rejection-sampled outside the user's positives."""
        rng = self._rng
        ptr, idx = self._net
        deg = np.diff(ptr)
        users = rng.integers(0, self.n_users, self.traindataSize)
        # a user without positives is skipped, and so is one without a free item: no negative exists for it, and
        # rk_bpr_sample answers valid = 0 for both
        users = users[(deg[users] > 0) & (deg[users] < self.n_items)]
        pos = idx[ptr[users] + (rng.random(len(users)) * deg[users]).astype(np.int64)]
        neg = rng.integers(0, self.n_items, len(users))
        todo = np.arange(len(users))
        while len(todo):
            keys = users[todo] * self.n_items + neg[todo]
            p = np.searchsorted(self._net_keys, keys)
            p = np.minimum(p, len(self._net_keys) - 1)
            clash = self._net_keys[p] == keys
            todo = todo[clash]
            neg[todo] = rng.integers(0, self.n_items, len(todo))
        return users.astype(np.int64), pos.astype(np.int64), neg.astype(np.int64)

    def pointwise_sample(self):
        """(user, item, label) rows as recad/dataset/implicit.py:77-91: every train positive
        plus negative_ratio*deg negatives per user drawn WITH replacement from the items the
        user has not interacted with in train."""
        rng = self._rng
        ptr, idx = self.train_csr_sorted()
        deg = np.diff(ptr)
        ratio = self.config["negative_ratio"]
        pu = np.repeat(np.arange(self.n_users, dtype=np.int64), deg)
        pi = idx.astype(np.int64)
        # a user who has interacted with every item has no negative to draw (the reference cannot draw one either):
        # it contributes its positives only
        nu = np.repeat(np.arange(self.n_users, dtype=np.int64), np.where(deg < self.n_items, deg * ratio, 0))
        # k-th free item of user u: draw a rank in the complement and skip over the sorted positives
        free = (self.n_items - deg)[nu]
        r = (rng.random(len(nu)) * free).astype(np.int64)
        # r-th free item of user u, exactly: idx[k] - k (k = position inside the user's sorted list) is the number
        # of free items below positive k and is non-decreasing, so j = #{k : idx[k] - k <= r} positives precede
        # the answer and the item is r + j (one vectorised binary search over per-user keys).
        k_in_row = np.arange(len(idx), dtype=np.int64) - np.repeat(ptr[:-1], deg)
        free_below = pu * self.n_items + (pi - k_in_row)          # sorted: user-major, non-decreasing inside a user
        j = np.searchsorted(free_below, nu * self.n_items + r, side="right") - ptr[nu]
        ni = r + j
        users = np.concatenate([pu, nu])
        items = np.concatenate([pi, ni])
        labels = np.concatenate([np.ones(len(pu), dtype=np.int64), np.zeros(len(nu), dtype=np.int64)])
        return users, items, labels

    def _device_epoch(self):
        """Samplers on the GPU (rk_bpr_sample / rk_pointwise_sample); shuffling by torch.randperm."""
        from . import _lib
        dev = torch.device(self.config["device"])
        seed = int(self._rng.integers(0, 2 ** 62))
        pairwise = self.config["sample"] == "pairwise"
        key = "_dev_net" if pairwise else "_dev_train"
        if not hasattr(self, key):
            ptr, idx = self._net if pairwise else self.train_csr_sorted()
            setattr(self, key, (torch.as_tensor(ptr, dtype=torch.int32).to(dev), torch.as_tensor(idx, dtype=torch.int32).to(dev)))
            # users without a free item (pointwise): rk_pointwise_sample writes (u, 0, label 0) for them, dropped below
            if not pairwise:
                full = np.diff(np.asarray(ptr)) >= self.n_items
                self._dev_full = torch.as_tensor(full).to(dev) if full.any() else None
        ptr, idx = getattr(self, key)
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed & 0x7FFFFFFF)
        if pairwise:
            n = self.traindataSize
            u, p, ng = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
            valid = torch.empty(n, dtype=torch.int32, device=dev)
            _lib.check(_lib.lib().rk_bpr_sample(self.n_users, self.n_items, _lib.ptr(ptr), _lib.ptr(idx), n, seed, _lib.ptr(u),
                                                _lib.ptr(p), _lib.ptr(ng), _lib.ptr(valid), _lib.stream_ptr()), "rk_bpr_sample")
            keep = valid.bool()
            cols = [t[keep] for t in (u, p, ng)]
            names, bs = ("users", "positive_items", "negative_items"), self.config["pairwise_batch_size"]
        else:
            ratio = self.config["negative_ratio"]
            E = idx.numel()
            n = E * (ratio + 1)
            cols = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3)]
            _lib.check(_lib.lib().rk_pointwise_sample(self.n_users, self.n_items, _lib.ptr(ptr), _lib.ptr(idx), E, ratio, seed,
                                                      _lib.ptr(cols[0]), _lib.ptr(cols[1]), _lib.ptr(cols[2]), _lib.stream_ptr()),
                       "rk_pointwise_sample")
            if self._dev_full is not None:
                keep = ~(self._dev_full[cols[0]] & (cols[2] == 0))
                cols = [c[keep] for c in cols]
            names, bs = ("users", "items", "labels"), self.config["pointwise_batch_size"]
        perm = torch.randperm(cols[0].numel(), device=dev, generator=gen)
        out = {k: c[perm].contiguous() for k, c in zip(names, cols)}
        out["batch_size"] = bs
        return out

    def generate_epoch(self):
        """One shuffled epoch as three int64 device tensors (+ batch size): the fast path the
        HIP victims consume; generate_batch() slices the same tensors."""
        dev = self.config["device"]
        smp = self.config["sampler"]
        if smp == "auto":
            smp = "device" if torch.device(dev).type == "cuda" else "numpy"
        if smp == "device" and self.config["sample"] in ("pairwise", "pointwise"):
            return self._device_epoch()
        if self.config["sample"] == "pairwise":
            cols, names, bs = self.pairwise_sample(), ("users", "positive_items", "negative_items"), self.config["pairwise_batch_size"]
        elif self.config["sample"] == "pointwise":
            cols, names, bs = self.pointwise_sample(), ("users", "items", "labels"), self.config["pointwise_batch_size"]
        else:
            raise NotImplementedError("Not implemented yet")
        perm = self._rng.permutation(len(cols[0]))
        out = {n: torch.from_numpy(c[perm]).to(dev) for n, c in zip(names, cols)}
        out["batch_size"] = bs
        return out

    def generate_batch(self, **config):
        if self._mode != "train":
            test = self.valid_dict if self._mode == "validate" else self.test_dict
            users = list(test.keys())
            bs = self.config["test_batch_size"]
            ap = self.allPos
            for i in range(0, len(users), bs):
                bu = users[i:i + bs]
                yield {"users": torch.tensor(bu, dtype=torch.int64, device=self.config["device"]),
                       "positive_items": [ap[u] for u in bu], "ground_truth": [test[u] for u in bu]}
            return
        ep = self.generate_epoch()
        bs = ep.pop("batch_size")
        n = len(next(iter(ep.values())))
        for i in range(0, n, bs):
            yield {k: v[i:i + bs] for k, v in ep.items()}

    # ------------------------------------------------------------------ perturbation
    def inject_data(self, data_mode, data, **kwargs):
        """recad/dataset/implicit.py:482-494 + fake_array2dict (:107-114): fake users are appended
        at ids n_users.., keeping the items rated STRICTLY above filter_num."""
        if data_mode != "explicit":
            raise NotImplementedError(f"Injection not supported in {data_mode} mode")
        assert len(data.shape) == 2, "Expect a user-item 2D rating matrix"
        uids, iids = np.where(np.asarray(data) > kwargs["filter_num"])
        ptr, idx = self._csr["train"]
        cnt = np.bincount(uids, minlength=data.shape[0])
        last = int(np.nonzero(cnt)[0].max()) + 1 if cnt.any() else 0
        new_ptr = np.concatenate([ptr, ptr[-1] + np.cumsum(cnt[:last])])
        order = np.argsort(uids, kind="stable")
        new_idx = np.concatenate([idx, iids[order].astype(np.int32)])
        return self.reset(train_csr=(new_ptr, new_idx), if_cache=False)

    def delete_data(self, data_mode, user_id, data, **kwargs):
        """recad/dataset/implicit.py:496-513: inject, then drop the flagged users."""
        ds = self.inject_data(data_mode, data, **kwargs)
        ptr, idx = ds._csr["train"]
        cnt = np.diff(ptr).copy()
        users = np.repeat(np.arange(len(cnt)), cnt)
        drop = np.isin(users, np.asarray(list(user_id)))
        cnt[np.asarray([u for u in user_id if u < len(cnt)], dtype=np.int64)] = 0
        new_ptr = np.zeros(len(cnt) + 1, dtype=np.int64)
        new_ptr[1:] = np.cumsum(cnt)
        return self.reset(train_csr=(new_ptr, idx[~drop]), if_cache=False)

    def partial_sample(self, **kwargs):
        assert "user_ratio" in kwargs, "Expect to have [user_ratio]"
        ratio = kwargs["user_ratio"]
        if abs(ratio - 1) < 1e-9:
            return self
        ptr, idx = self._csr["train"]
        users = [u for u in range(self.n_users) if ptr[u + 1] > ptr[u]]
        random.shuffle(users)
        keep = np.zeros(self.n_users, dtype=bool)
        keep[users[: int(len(users) * ratio)]] = True
        cnt = np.diff(ptr) * keep
        mask = np.repeat(keep, np.diff(ptr))
        new_ptr = np.zeros(self.n_users + 1, dtype=np.int64)
        new_ptr[1:] = np.cumsum(cnt)
        return self.reset(train_csr=(new_ptr, idx[mask]))

    def print_help(self, **kwargs):
        from pprint import pprint

        pprint({**self.info_describe(), "dataset_name": self.dataset_name})


# ---------------------------------------------------------------------------------------------- explicit feedback
def _coo_to_rating_csr(users, items, ratings, n_rows):
    """(ptr int64 [n_rows + 1], idx int32, val float32): rows sorted by item, duplicate (user, item) ratings summed --
    what csr_matrix((rating, (row, col))).toarray() holds (explicit.py:125-134)."""
    users = np.asarray(users, dtype=np.int64)
    items = np.asarray(items, dtype=np.int64)
    ratings = np.asarray(ratings, dtype=np.float32)
    width = int(items.max()) + 1 if len(items) else 1
    keys = users * width + items
    uniq, inv = np.unique(keys, return_inverse=True)
    val = np.zeros(len(uniq), dtype=np.float32)
    np.add.at(val, inv, ratings)
    cnt = np.bincount(uniq // width, minlength=n_rows)[:n_rows] if len(uniq) else np.zeros(n_rows, dtype=np.int64)
    ptr = np.zeros(n_rows + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(cnt)
    return ptr, (uniq % width).astype(np.int32), val


def _canonical_rating_csr(csr):
    """A caller's (ptr, idx, val) with every row sorted by item and duplicates summed (unchanged when it already is)."""
    ptr, idx, val = (np.asarray(a) for a in csr[:3])
    ptr = ptr.astype(np.int64)
    idx = idx.astype(np.int32)
    val = val.astype(np.float32)
    if len(idx) != int(ptr[-1]) or len(val) != len(idx):
        raise ValueError(f"rating CSR sizes disagree: ptr[-1] = {int(ptr[-1])}, {len(idx)} ids, {len(val)} values")
    n = len(ptr) - 1
    users = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    width = int(idx.max()) + 1 if len(idx) else 1
    keys = users * width + idx.astype(np.int64)
    if len(keys) > 1 and not bool(np.all(keys[1:] > keys[:-1])):
        return _coo_to_rating_csr(users, idx, val, n)
    return ptr, idx, val


def _rows_of(csr, n_rows):
    ptr, idx, val = csr
    if len(ptr) - 1 >= n_rows:
        return ptr[: n_rows + 1], idx[: int(ptr[n_rows])], val[: int(ptr[n_rows])]
    out = np.full(n_rows + 1, ptr[-1], dtype=np.int64)
    out[: len(ptr)] = ptr
    return out, idx, val


def _kvr_of(csr):
    ptr, idx, val = csr
    users = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    return np.column_stack([users.astype(np.float64), idx.astype(np.float64), val.astype(np.float64)])


def read_rating_csv(path, header=None, sep=","):
    """explicit.py:110-120: the columns ['user_id', 'item_id', 'rating'] of a CSV as an [N, 3] array."""
    import pandas as pd

    header = header if header is not None else ["user_id", "item_id", "rating"]
    return pd.read_csv(path, engine="python", sep=sep).loc[:, header].to_numpy()


class ExplicitData:
    """Explicit-feedback (rating) dataset: the build's counterpart of recad/dataset/explicit.py.

    Same object contract -- ``info_describe()`` (n_users, n_items, *_interactions, train_kvr, train_mat,
    batch_describe, user_map after a remap), ``generate_batch(user_filter=)``, ``partial_sample``, ``reset`` -- but the
    ratings live in CSR arrays (duplicates summed, rows sorted by item).  The reference's dense U x I ``train_mat``
    (explicit.py:102) is built only on first access and refused above ``dense_limit`` entries; the AUSH attacker never
    asks for it.  Sources, per split: ``*_csr=(ptr, idx, val)``, the reference's ``*_dict`` [N, 3] (user, item, rating)
    arrays, or its CSVs (``path_*``).  A missing valid / test split is empty; a missing train split is an error (there
    is no download)."""

    def __init__(self, **config):
        self.config = config
        self.logger = get_logger(f"{__name__}:{self.dataset_name}", level=config["logging_level"])
        self._mode = "train"
        self._kvr = {}
        coo = {}
        for split in ("train", "valid", "test"):
            if config.get(f"{split}_csr") is not None:
                coo[split] = ("csr", _canonical_rating_csr(config[f"{split}_csr"]))
            elif config.get(f"{split}_dict") is not None:
                kvr = np.asarray(config[f"{split}_dict"])
                self._kvr[split] = kvr
                coo[split] = ("kvr", kvr)
            elif config.get(f"path_{split}"):
                kvr = read_rating_csv(config[f"path_{split}"], config["header"], config["sep"])
                self._kvr[split] = kvr
                coo[split] = ("kvr", kvr)
            elif split == "train":
                raise ValueError(f"ExplicitData({self.dataset_name}): no train split -- give train_csr=(ptr, idx, val), "
                                 "train_dict=[N, 3] (user, item, rating) rows or path_train=<csv>; there is no download")
            else:
                coo[split] = ("kvr", np.zeros((0, 3)))
                self._kvr[split] = coo[split][1]
        self.user_map = config.get("user_map")
        if config["remap_enable"] and self.user_map is None:
            # explicit.py:71-81: users of the three splits renumbered densely in sorted order
            ids = [np.repeat(np.arange(len(d[0]) - 1), np.diff(d[0])) if kind == "csr" else d[:, 0].astype(np.int64)
                   for kind, d in coo.values()]
            uniq = np.unique(np.concatenate(ids)) if ids else np.zeros(0, dtype=np.int64)
            self.user_map = {int(u): i for i, u in enumerate(uniq)}
            remap = np.full(int(uniq.max()) + 1 if len(uniq) else 1, -1, dtype=np.int64)
            remap[uniq] = np.arange(len(uniq))
            for split, (kind, d) in list(coo.items()):
                if kind == "kvr":
                    d = d.copy()
                    d[:, 0] = remap[d[:, 0].astype(np.int64)]
                    self._kvr[split] = d
                    coo[split] = ("kvr", d)
                else:
                    ptr, idx, val = d
                    users = remap[np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))]
                    coo[split] = ("csr", _coo_to_rating_csr(users, idx, val, len(uniq)))
        # n_users / n_items = max id + 1 over train, valid and test (explicit.py:83-100)
        def extent(kind, d):
            if kind == "kvr":
                return ((int(d[:, 0].max()) + 1, int(d[:, 1].max()) + 1) if len(d) else (0, 0))
            ptr, idx, _ = d
            rows = np.nonzero(np.diff(ptr))[0]
            return (int(rows.max()) + 1 if len(rows) else 0, int(idx.max()) + 1 if len(idx) else 0)

        ext = [extent(*v) for v in coo.values()]
        self.n_users = max(e[0] for e in ext)
        self.n_items = max(e[1] for e in ext)
        self._csr = {}
        sizes = {}
        for split, (kind, d) in coo.items():
            if kind == "kvr":
                self._csr[split] = _coo_to_rating_csr(d[:, 0], d[:, 1], d[:, 2], self.n_users) if len(d) else \
                    (np.zeros(self.n_users + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
                sizes[split] = len(d)
            else:
                self._csr[split] = _rows_of(d, self.n_users)
                sizes[split] = int(self._csr[split][0][-1])
        self.train_size, self.valid_size, self.test_size = sizes["train"], sizes["valid"], sizes["test"]
        self._train_mat = None

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_config(cls, name, **user_config):
        config = {k: copy(v) for k, v in DATASET_EXPLICIT.items()}
        for k, v in user_config.items():
            if k == "download":
                continue
            if k not in config:
                get_logger(__name__).debug(f"Unexpected key [{k}] for {cls}")
            config[k] = v
        inst = object.__new__(cls)
        inst._dataset_name = name
        inst._init_config = config
        inst.__init__(**config)
        return inst

    @property
    def dataset_name(self):
        return getattr(self, "_dataset_name", type(self).__name__)

    def reset(self, **kwargs):
        config = copy(self._init_config)
        for k, v in kwargs.items():
            if k not in config:
                raise ValueError(f"reset arg {k} should be in {list(config)}")
            config[k] = v
            if k.endswith("_dict") and v is not None:
                config[k.replace("_dict", "_csr")] = None
            if k.endswith("_csr") and v is not None:
                config[k.replace("_csr", "_dict")] = None
        return type(self).from_config(self.dataset_name, **config)

    # ------------------------------------------------------------------ description
    def rating_csr(self, split="train"):
        """(ptr int64 [n_users + 1], idx int32, val float32) of a split: rows sorted by item, duplicates summed."""
        return self._csr[split]

    @property
    def train_kvr(self):
        if "train" not in self._kvr:
            self._kvr["train"] = _kvr_of(self._csr["train"])
        return self._kvr["train"]

    @property
    def train_mat(self):
        """The dense U x I float32 rating array of the reference (explicit.py:102), built on first access."""
        if self._train_mat is None:
            n = self.n_users * self.n_items
            if n > self.config["dense_limit"]:
                raise MemoryError(f"ExplicitData.train_mat: a dense {self.n_users} x {self.n_items} array ({n * 4 / 2 ** 30:.1f} GiB) "
                                  f"is above dense_limit = {self.config['dense_limit']} entries; use rating_csr() instead")
            ptr, idx, val = self._csr["train"]
            mat = np.zeros((self.n_users, self.n_items), dtype=np.float32)
            mat[np.repeat(np.arange(self.n_users), np.diff(ptr)), idx] = val
            self._train_mat = mat
        return self._train_mat

    def batch_describe(self):
        if self._mode == "train":
            b = VarDim(max=self.config["batch_size"], comment="batch size")
            return {"users": (torch.int64, b), "users_mat": (torch.float32, (b, self.n_items))}

    class _Info(dict):
        """info_describe() result; train_kvr / train_mat are materialised on first access."""

        def __init__(self, ds, base):
            super().__init__(base)
            self._ds = ds

        def __missing__(self, key):
            if key not in ("train_kvr", "train_mat"):
                raise KeyError(key)
            self[key] = getattr(self._ds, key)
            return self[key]

        def get(self, key, default=None):
            try:
                return self[key]
            except KeyError:
                return default

        def keys(self):
            return list(super().keys()) + [k for k in ("train_kvr", "train_mat") if not dict.__contains__(self, k)]

        def __contains__(self, key):
            return dict.__contains__(self, key) or key in ("train_kvr", "train_mat")

    def info_describe(self):
        base = {"n_users": self.n_users, "n_items": self.n_items, "train_interactions": self.train_size,
                "valid_interactions": self.valid_size, "test_interactions": self.test_size,
                "batch_describe": self.batch_describe()}
        if self.user_map is not None:
            base["user_map"] = self.user_map
        return ExplicitData._Info(self, base)

    def mode(self):
        return self._mode

    def switch_mode(self, mode):
        assert mode in ["train", "test", "validate"]
        self._mode = mode

    def _dense_rows(self, users):
        ptr, idx, val = self._csr["train"]
        out = np.zeros((len(users), self.n_items), dtype=np.float32)
        for r, u in enumerate(users):
            out[r, idx[ptr[u]:ptr[u + 1]]] = val[ptr[u]:ptr[u + 1]]
        return out

    def generate_batch(self, **config):
        """explicit.py:178-199: a permutation (np.random) of the users user_filter(train_mat=...) returns (all users without
        a filter) in batches of batch_size, each with its dense rating rows."""
        if self._mode != "train":
            return
        user_filter = config.get("user_filter", None)
        bs = self.config["batch_size"]
        avail = user_filter(train_mat=self.train_mat) if user_filter is not None else list(range(self.n_users))
        avail = np.random.permutation(avail)
        dev = self.config["device"]
        for b in range((len(avail) + bs - 1) // bs):
            users = avail[b * bs:(b + 1) * bs]
            yield {"users": torch.tensor(users, dtype=torch.int64).to(dev),
                   "users_mat": torch.tensor(self._dense_rows(users), dtype=torch.float32).to(dev)}

    def inject_data(self, mode, data, **kwargs):
        raise NotImplementedError("ExplicitData.inject_data: not supported (the reference's explicit dataset has none either)")

    def delete_data(self, mode, user_id, data, **kwargs):
        raise NotImplementedError("ExplicitData.delete_data: not supported (the reference's explicit dataset has none either)")

    def partial_sample(self, **kwargs):
        """explicit.py:210-240: np.random.shuffle the unique train users, keep int(len * user_ratio) of them in every split
        and renumber them densely in sorted order (user_map); item ids are kept, so n_items may shrink."""
        assert "user_ratio" in kwargs, "Expect to have [user_ratio]"
        ratio = kwargs["user_ratio"]
        ptr = self._csr["train"][0]
        users = np.nonzero(np.diff(ptr))[0]
        np.random.shuffle(users)
        left = np.sort(users[: int(len(users) * ratio)])
        new_map = {int(u): k for k, u in enumerate(left.tolist())}
        splits = {}
        for split in ("train", "valid", "test"):
            p, i, v = self._csr[split]
            cnt = np.diff(p)[left]
            np_ = np.zeros(len(left) + 1, dtype=np.int64)
            np_[1:] = np.cumsum(cnt)
            sel = np.concatenate([np.arange(p[u], p[u + 1]) for u in left]) if len(left) else np.zeros(0, dtype=np.int64)
            splits[split] = (np_, i[sel], v[sel])
        return self.reset(train_csr=splits["train"], valid_csr=splits["valid"], test_csr=splits["test"], remap_enable=True,
                          user_map=new_map, if_cache=False)

    def print_help(self, **kwargs):
        from pprint import pprint

        pprint({**self.info_describe(), "dataset_name": self.dataset_name})


factories = {"implicit": ImplicitData, "explicit": ExplicitData}


def from_config(scope, *args, **kwargs):
    """dataset.from_config("implicit" | "explicit", name, **kw) (recad/dataset/__init__.py:13-17)."""
    return factories[scope].from_config(*args, **kwargs)
