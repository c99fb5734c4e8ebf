"""What the attackers' ``_build``s share: the attack data as a rating CSR, the opening of ``_build`` and the template draw of
the two surrogate attackers."""
import numpy as np
import torch

from .. import _lib
from ..utils import get_logger


def train_csr(ds):
    """(n_users, n_items, ptr, idx, val) of the attack data: an ExplicitData's rating CSR, or the dense train_mat of a
    foreign dataset with the reference's info_describe()."""
    if hasattr(ds, "rating_csr"):
        ptr, idx, val = ds.rating_csr("train")
        return int(ds.n_users), int(ds.n_items), ptr, idx, val
    info = ds.info_describe()
    mat = np.asarray(info["train_mat"], dtype=np.float32)
    nz = mat != 0
    ptr = np.zeros(mat.shape[0] + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(nz.sum(axis=1))
    return int(mat.shape[0]), int(mat.shape[1]), ptr, np.nonzero(nz)[1].astype(np.int32), mat[nz]


def need_dataset(attacker, config):
    """The dataset handed to .I(); an attacker built without one is refused by its class name."""
    ds = config.get("dataset")
    if ds is None:
        raise ValueError(f"{type(attacker).__name__} needs dataset= (an explicit dataset) at .I()")
    return ds


def open_build(attacker, config):
    """The opening of every attacker's _build: the dataset, a HIP device or a loud failure, then the logger, the device and
    the attack data.  Returns (dataset, n_users, n_items, ptr, idx, val).  A _build that refuses settings before it asks for
    a device calls need_dataset and its own checks first."""
    ds = need_dataset(attacker, config)
    _lib.require_gpu()
    attacker.logger = get_logger(type(attacker).__module__, level=config.get("logging_level", 20))
    attacker.device = torch.device(config.get("device", "cuda"))
    return (ds,) + train_csr(ds)


def draw_templates(ptr, idx, val, attack_num, filler_num, need_filler_num):
    """build_network's draws on a rating CSR: np.random.choice of attack_num template users -- among those with at least
    filler_num positive ratings when need_filler_num (aia.py:54-63), else among all users (aushplus.py:24-30) -- then per
    template one np.random.shuffle of its nonzero columns, the first filler_num kept.  Returns (users [attack_num], list of
    the kept columns per template in shuffle order)."""
    ptr, idx, val = np.asarray(ptr), np.asarray(idx), np.asarray(val)
    n_users = len(ptr) - 1
    if need_filler_num:
        rows = np.repeat(np.arange(n_users), np.diff(ptr))
        cnt = np.bincount(rows[val > 0], minlength=n_users)      # np.sum(train_array > 0, 1)
        pool = np.where(cnt >= filler_num)[0]
    else:
        pool = range(n_users)
    users = np.random.choice(pool, attack_num)
    kept = []
    for u in users:
        b, e = ptr[u], ptr[u + 1]
        fillers = idx[b:e][val[b:e] != 0].astype(np.int64)
        np.random.shuffle(fillers)
        kept.append(fillers[:filler_num].copy())
    return users, kept
