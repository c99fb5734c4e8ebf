"""PCASelectUsers: spectral fake-user detection on the device.

The reference's only defender (recad/model/defense/PCASelectUsers.py, registry recad/default.py:223-228) builds
a dense U x I rating array A, z-scores its columns without centring (sklearn ``scale(axis=0, with_mean=False)``),
takes the k largest eigenpairs of the I x I matrix C = S^T S with ARPACK, scores every user by
``sum_j ((A o A) . v_j)[u]`` and flags the ``attack_num / U * U`` users of smallest score.

Here nothing dense is formed: C.X = D^-1 A^T (A (D^-1 X)) is two narrow SpMMs over the rating CSR and its
transpose (rk_pca_spmm), and the eigenpairs come from block subspace iteration with Rayleigh-Ritz.  Every O(nnz)
and O(I*b) step runs in HIP (csrc/pca.hip); only b x b fp64 matrices travel to the host, once per iteration.

Sign convention (the one deliberate departure from the reference, whose ARPACK signs are arbitrary): every
eigenvector is flipped so that its entry of largest magnitude is positive, the lowest index winning a tie.
"""
import numpy as np
import torch

from .. import _lib
from .._ratings import rating_csr  # noqa: F401  (callers import it from here as well)
from ._select_users import SelectUsersDefender, flag_count  # noqa: F401  (flag_count: callers import it from here as well)


def effective_k(k, n_users, n_items):
    """PCASelectUsers.py:30-32: kVals >= min(U, I) falls back to 3."""
    return 3 if k >= min(n_users, n_items) else int(k)


def block_width(k):
    """Width b of the iteration block for k wanted eigenpairs: 8 up to k = 3, 16 from k = 4 to 16.  The b - k guard vectors set
    the convergence rate lambda_{b+1} / lambda_k; with b = 8, k = 5 leaves three guards and the reference's dev data (lambda_5
    and lambda_6 0.14 % apart, lambda_9 / lambda_5 = 0.977) does not reach tol in 300 iterations, k = 4 needs 240 of them
    (DESIGN.md section 9).  k = 3 keeps the width it has always had.  Above 16 no supported width holds k."""
    k = int(k)
    if k < 1 or k > 16:
        raise ValueError(f"kVals = {k}: the solver's block holds 1 to 16 eigenpairs (block width 8 or 16)")
    return 8 if k <= 3 else 16


def sign_fix(vecs):
    """The sign convention: column j is negated unless its entry of largest |value| (lowest index on a tie) is positive.
    numpy (host) or torch (any device) arrays of shape [n, k]."""
    if isinstance(vecs, torch.Tensor):
        pos = vecs.abs().argmax(dim=0)
        s = torch.sign(vecs.gather(0, pos.view(1, -1))).view(-1)
        return vecs * torch.where(s == 0, torch.ones_like(s), s)
    vecs = np.asarray(vecs)
    pos = np.argmax(np.abs(vecs), axis=0)
    s = np.sign(vecs[pos, np.arange(vecs.shape[1])])
    return vecs * np.where(s == 0, 1, s)


class CovarianceOperator:
    """C = D^-1 A^T A D^-1 (PCASelectUsers.py:60-64) applied to [I, b] row-major fp32 blocks, on the device."""

    def __init__(self, U, I, rowptr, col, val):
        self.U, self.I, self.rowptr, self.col, self.val = U, I, rowptr, col, val
        dev = val.device
        nnz = col.numel()
        self.t_rowptr = torch.empty(I + 1, dtype=torch.int32, device=dev)
        self.t_col = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        self.t_val = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)
        self.inv_scale = torch.empty(I, dtype=torch.float32, device=dev)
        self.sigma = torch.empty(I, dtype=torch.float32, device=dev)
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
        _lib.check(L.rk_pca_transpose(U, I, P(rowptr), P(col), P(val), P(self.t_rowptr), P(self.t_col), P(self.t_val), s), "rk_pca_transpose")
        _lib.check(L.rk_pca_col_scale(I, U, P(self.t_rowptr), P(self.t_val), P(self.inv_scale), P(self.sigma), s), "rk_pca_col_scale")
        self._tmp = {}

    def apply(self, X, Y):
        """Y = C X for X, Y [I, b] (b in {8, 16})."""
        b = X.shape[1]
        T = self._tmp.get(b)
        if T is None:
            T = self._tmp[b] = torch.empty(self.U, b, dtype=torch.float32, device=X.device)
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(X.device)
        _lib.check(L.rk_pca_spmm(self.U, P(self.rowptr), P(self.col), P(self.val), P(self.inv_scale), None, b, P(X), P(T), s), "rk_pca_spmm")
        _lib.check(L.rk_pca_spmm(self.I, P(self.t_rowptr), P(self.t_col), P(self.t_val), None, P(self.inv_scale), b, P(T), P(Y), s),
                   "rk_pca_spmm")
        return Y


class _Block:
    """Device helpers of the solver: fp64 Gram and V . M (csrc/pca.hip)."""

    def __init__(self, n, dev):
        self.n, self.dev = n, dev
        self.part = torch.empty(_lib.RK_PCA_GRAM_BLOCKS * 32 * 32, dtype=torch.float64, device=dev)
        self.G = torch.empty(32 * 32, dtype=torch.float64, device=dev)

    def gram(self, P_, Q_=None):
        p, q = P_.shape[1], (0 if Q_ is None else Q_.shape[1])
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(self.dev)
        _lib.check(L.rk_pca_gram(self.n, P(P_), p, P(Q_), q, P(self.part), P(self.G), s), "rk_pca_gram")
        w = p + q
        return self.G[: w * w].cpu().numpy().reshape(w, w).copy()

    def update(self, V, M, out):
        M_d = torch.from_numpy(np.ascontiguousarray(M, dtype=np.float64)).to(self.dev)
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(self.dev)
        _lib.check(L.rk_pca_update(self.n, P(V), V.shape[1], P(M_d), M.shape[1], P(out), s), "rk_pca_update")
        return out

    @staticmethod
    def _chol_inv(G):
        try:
            return np.linalg.inv(np.linalg.cholesky(G).T)
        except np.linalg.LinAlgError:     # numerically rank-deficient block: the symmetric inverse square root instead
            s, U_ = np.linalg.eigh(G)
            return U_ / np.sqrt(np.maximum(s, s.max() * 1e-14))

    def orth(self, Y, tmp):
        """CholQR2 in place: Y <- Y R1^-1 R2^-1, R from the Cholesky factor of the fp64 Gram (host, b x b); tmp is
        scratch of Y's shape."""
        self.update(Y, self._chol_inv(self.gram(Y)), tmp)
        self.update(tmp, self._chol_inv(self.gram(tmp)), Y)
        return Y


def subspace_eigs(op, k, b, tol=1e-5, max_iter=300, seed=2023):
    """The k largest eigenpairs of the PSD operator `op` (CovarianceOperator) by block subspace iteration with
    Rayleigh-Ritz, block width b.  Stops when ||C v_j - lambda_j v_j|| <= tol * lambda_1 for every j < k (residual
    norms from the fp64 Gram of [V | CV]); raises RuntimeError naming the residuals after max_iter applications of C.
    Returns (eigenvalues float64 [k] descending, eigenvectors fp32 device [I, k] (sign convention applied), iterations,
    residuals)."""
    n, dev = op.I, op.val.device
    if b not in (8, 16) or k > b or k < 1:
        raise ValueError(f"block width {b} (key `block`) must be 8 or 16 and at least kVals = {k} >= 1")
    if n < b:
        raise ValueError(f"{n} items: fewer than the block width {b}")
    blk = _Block(n, dev)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    V = torch.randn(n, b, generator=gen, dtype=torch.float32).to(dev)
    tmp, W = torch.empty_like(V), torch.empty_like(V)
    blk.orth(V, tmp)
    lam = res = None
    for it in range(1, int(max_iter) + 1):
        op.apply(V, W)
        G = blk.gram(V, W)
        VV, VW, WW = G[:b, :b], G[:b, b:], G[b:, b:]
        H = 0.5 * (VW + VW.T)
        # generalised Ritz problem H q = lam VV q (VV = I up to fp32 rounding of V)
        try:
            Li = np.linalg.inv(np.linalg.cholesky(VV))
        except np.linalg.LinAlgError as e:
            # CholQR2 leaves V orthonormal to fp32 rounding whenever its input had b independent columns: this can fail only
            # when C has numerically fewer than b nonzero eigenvalues
            raise RuntimeError(f"PCASelectUsers: the iteration block lost rank in iteration {it} (block {b}, k {k}): the scaled "
                               f"rating matrix has fewer than {b} independent columns") from e
        lam_all, Z = np.linalg.eigh(Li @ H @ Li.T)
        order = np.argsort(-lam_all, kind="stable")
        lam_all, Q = lam_all[order], (Li.T @ Z)[:, order]
        r2 = (np.einsum("ij,ik,kj->j", Q, WW, Q) - 2 * lam_all * np.einsum("ij,ik,kj->j", Q, VW, Q)
              + lam_all ** 2 * np.einsum("ij,ik,kj->j", Q, VV, Q))
        res = np.sqrt(np.maximum(r2, 0.0))
        lam = lam_all
        if lam[0] > 0 and np.all(res[:k] <= tol * lam[0]):
            out = torch.empty(n, k, dtype=torch.float32, device=dev)
            blk.update(V, Q[:, :k], out)
            return lam[:k].copy(), sign_fix(out).contiguous(), it, res[:k].copy()
        # next basis: orth(C V Q diag(1 / lambda)) -- the Ritz images, scaled to comparable norms for CholQR2
        scale = np.where(lam_all > 0, 1.0 / np.where(lam_all > 0, lam_all, 1.0), 1.0)
        blk.update(W, Q * scale[None, :], V)
        blk.orth(V, tmp)
    raise RuntimeError(f"PCASelectUsers: subspace iteration did not converge in {max_iter} iterations (block {b}, k {k}): "
                       f"residuals / lambda_1 = {[float(r) for r in (res[:k] / lam[0])]} > tol {tol}")


class PCASelectUsers(SelectUsersDefender):
    """Lazy like the reference, through SelectUsersDefender: ``model.from_config("defender", "PCASelectUsers", kVals=3,
    attack_num=50)`` keeps the configuration, ``.I(dataset=...)`` builds it, ``defense_step()`` returns the flagged user ids.
    Afterwards ``eigenvalues``, ``eigenvectors``, ``distances``, ``predLabels`` and ``disSort`` hold what the reference's
    attributes hold (eigenvectors / distances as device tensors)."""

    victim_name = "PCASelectUsers"

    def _build(self, kVals, attack_num, block, tol, max_iter, seed, **config):
        self.kVals, self.attack_num = int(kVals), int(attack_num)
        self.block, self.tol, self.max_iter, self.seed = block, float(tol), int(max_iter), int(seed)
        self.eigenvalues = self.eigenvectors = self.distances = self.predLabels = None
        self.iterations = 0
        self._open(config)

    def _detect(self, U, I, rowptr, col, val):
        """PCASelectUsers.py:47-93 on the device."""
        if val.numel() and not bool(torch.isfinite(val).all().item()):
            raise ValueError("PCASelectUsers: the rating matrix holds non-finite values")
        k = effective_k(self.kVals, U, I)
        if k != self.kVals:
            self.logger.info(f"k-vals is more than the number of user or item, so it is set to {k}")
        b = int(self.block) if self.block else block_width(k)
        op = CovarianceOperator(U, I, rowptr, col, val)
        self.k = k
        self.eigenvalues, self.eigenvectors, self.iterations, self.residuals = subspace_eigs(
            op, k, b, tol=self.tol, max_iter=self.max_iter, seed=self.seed)
        L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(self.device)
        w = torch.empty(I, dtype=torch.float32, device=self.device)
        dist = torch.empty(U, dtype=torch.float32, device=self.device)
        _lib.check(L.rk_pca_sq_spmv(U, I, P(rowptr), P(col), P(val), P(self.eigenvectors), k, k, P(w), P(dist), s), "rk_pca_sq_spmv")
        order = torch.empty(U, dtype=torch.int32, device=self.device)
        _lib.check(L.rk_pca_select(U, P(dist), U, P(order), s), "rk_pca_select")
        self.distances = dist
        self.testLabels = np.zeros(U)
        return self._flag(order, U)

    @property
    def disSort(self):
        """[(user id, distance)] in ascending distance, ties to the lower id (PCASelectUsers.py:80), built on first use."""
        return self._pairs(self.distances)
