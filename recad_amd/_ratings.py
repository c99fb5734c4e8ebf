"""The U x I rating matrix as the item-item victims, iALS and the defenders read it: the device CSR of a dataset
(``rating_csr``), the same cached per device and checked against the dataset's description (``DeviceRatings``), the validation
every one of them starts with (``checked_norms``: rk_knn_norms, with its refusal as a ValueError) and the transpose
(``transposed``: rk_pca_transpose)."""
import numpy as np
import torch

from . import _lib


def rating_csr(dataset, device):
    """The U x I rating matrix as a device CSR: (U, I, rowptr int32, col int32, val float32).
    Accepts an ImplicitData (its train CSR, every value 1.0), a rating CSR tuple (ptr, idx, val[, n_items]),
    a dense U x I array (the reference's users_mat rows), or an object whose info_describe() has "train_mat".
    An ExplicitData gives its train rating CSR, values as they are (the reference's defense_data, explicit.py:102)."""
    from .dataset import ExplicitData

    if isinstance(dataset, ExplicitData):
        ptr, idx, val = dataset.rating_csr("train")
        return (int(dataset.n_users), int(dataset.n_items), torch.as_tensor(ptr.astype(np.int32)).to(device),
                torch.as_tensor(idx.astype(np.int32)).to(device), torch.as_tensor(val.astype(np.float32)).to(device))
    if hasattr(dataset, "train_csr_sorted") and hasattr(dataset, "n_items"):
        ptr, idx = dataset.train_csr_sorted()
        U, I = int(dataset.n_users), int(dataset.n_items)
        ptr, idx = np.asarray(ptr)[: U + 1], np.asarray(idx)[: int(ptr[U])]
        rp = torch.as_tensor(ptr.astype(np.int32)).to(device)
        col = torch.as_tensor(idx.astype(np.int32)).to(device)
        return U, I, rp, col, torch.ones(col.numel(), dtype=torch.float32, device=device)
    if hasattr(dataset, "info_describe") and not isinstance(dataset, (tuple, list)):
        dataset = dataset.info_describe()["train_mat"]
    if isinstance(dataset, (tuple, list)):
        if len(dataset) not in (3, 4):
            raise ValueError("a rating CSR is (ptr, idx, val) or (ptr, idx, val, n_items)")
        ptr, idx, val = (torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a) for a in dataset[:3])
        U = int(ptr.numel()) - 1
        I = int(dataset[3]) if len(dataset) == 4 else (int(idx.max().item()) + 1 if idx.numel() else 1)
        if idx.numel() != int(ptr[-1].item()) or val.numel() != idx.numel():
            raise ValueError(f"rating CSR sizes disagree: ptr[-1] = {int(ptr[-1].item())}, {idx.numel()} ids, {val.numel()} values")
        if idx.numel() and (int(idx.min().item()) < 0 or int(idx.max().item()) >= I):
            raise ValueError(f"rating CSR item ids outside [0, {I})")
        if int(ptr[0].item()) != 0 or bool((ptr[1:] < ptr[:-1]).any().item()):
            raise ValueError("rating CSR row pointers must start at 0 and not decrease")
        return (U, I, ptr.to(device=device, dtype=torch.int32).contiguous(), idx.to(device=device, dtype=torch.int32).contiguous(),
                val.to(device=device, dtype=torch.float32).contiguous())
    dense = torch.as_tensor(np.asarray(dataset) if not isinstance(dataset, torch.Tensor) else dataset)
    if dense.dim() != 2:
        raise ValueError(f"expected a U x I rating array, got shape {tuple(dense.shape)}")
    dense = dense.to(device=device, dtype=torch.float32)
    U, I = dense.shape
    mask = dense != 0
    rp = torch.zeros(U + 1, dtype=torch.int32, device=device)
    rp[1:] = torch.cumsum(mask.sum(dim=1), 0).to(torch.int32)
    nz = mask.nonzero()
    return int(U), int(I), rp, nz[:, 1].to(torch.int32).contiguous(), dense[mask].contiguous()


class DeviceRatings:
    """A victim's view of its dataset's rating matrix: loaded on first use and kept for that device."""

    def __init__(self, dataset, n_users, n_items, who):
        self.dataset, self.shape, self.who = dataset, (n_users, n_items), who
        self._csr = None                  # (device, rowptr, col, val)

    def on(self, dev):
        """(rowptr, col, val) on `dev`.  A matrix that is not of the described shape is a ValueError."""
        if self._csr is None or self._csr[0] != dev:
            U, I, rowptr, col, val = rating_csr(self.dataset, dev)
            if (U, I) != self.shape:
                raise ValueError(f"{self.who}: the dataset's rating matrix is {U} x {I}, its description says "
                                 f"{self.shape[0]} x {self.shape[1]}")
            if col.numel() == 0:          # an empty matrix still needs addresses
                col, val = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.float32, device=dev)
            self._csr = (dev, rowptr, col, val)
        return self._csr[1:]


def checked_norms(who, what, n_rows, n_cols, rowptr, col, val):
    """rk_knn_norms of the CSR -> the reciprocal row norms, fp32 [n_rows].  A refusal raises ValueError naming the rule and the
    row, and nothing further is launched; the status words are read only then."""
    dev = val.device
    L, P = _lib.lib(), _lib.ptr
    rnorm = torch.empty(n_rows, dtype=torch.float32, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    bad = device_refusal(L.rk_knn_norms(n_rows, n_cols, P(rowptr), P(col), P(val), P(rnorm), P(status), _lib.stream_ptr(dev)),
                         "rk_knn_norms", status)
    if bad:
        raise ValueError(f"{who}: the {what} breaks rule {bad[0]} ({_lib.RK_KNN_RULES.get(bad[0], '?')}), first in row {bad[1]}")
    return rnorm


def device_refusal(rc, what, status):
    """(rule, index) of a device refusal read from the entry point's status words, None when the call succeeded; any other
    failure raises HipCallError."""
    if rc == 0:
        return None
    rule, index = status.cpu().tolist()
    if not rule:
        _lib.check(rc, what)
    return rule, index


def transposed(n_rows, n_cols, rowptr, col, val):
    """rk_pca_transpose -> (colptr int32 [n_cols + 1], crow int32, cval fp32): the rows of the transpose, ascending."""
    dev = val.device
    L, P = _lib.lib(), _lib.ptr
    nnz = max(int(col.numel()), 1)
    colptr = torch.empty(n_cols + 1, dtype=torch.int32, device=dev)
    crow = torch.empty(nnz, dtype=torch.int32, device=dev)
    cval = torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.check(L.rk_pca_transpose(n_rows, n_cols, P(rowptr), P(col), P(val), P(colptr), P(crow), P(cval), _lib.stream_ptr(dev)),
               "rk_pca_transpose")
    return colptr, crow, cval
