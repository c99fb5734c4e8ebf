"""A numpy restatement of recad_amd.defense.pca_select_users.subspace_eigs for CPU tests: the same start block, the
same CholQR2, Rayleigh-Ritz step and stopping rule, in fp64 arithmetic with V, T and W rounded to fp32 after each
product (what the device stores).  The operator is a callable X [n, b] -> C X.  It predicts iteration counts of the
device solver closely enough to keep the block-width rule honest without a GPU; it is not the product."""
import numpy as np
import torch


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _csr_mm(ptr, idx, val, X):
    """CSR times dense in fp64 (rows summed in storage order); empty rows give zeros."""
    out = np.zeros((len(ptr) - 1, X.shape[1]))
    live = np.diff(ptr) > 0
    if live.any():
        out[live] = np.add.reduceat(val[:, None] * X[idx], ptr[:-1][live], axis=0)
    return out


def golden_operator(g):
    """C = D^-1 A^T A D^-1 of a pca_*.npz fixture as a callable on [I, b] blocks, plus (U, I).  D by the defender's rule:
    population variance over all U rows, below 10 * FLT_EPSILON in fp32 counts as constant (scale 1)."""
    U, I = int(g["n_users"]), int(g["n_items"])
    ptr, idx, val = g["ptr"].astype(np.int64), g["idx"].astype(np.int64), g["val"].astype(np.float64)
    rows = np.repeat(np.arange(U), np.diff(ptr))
    order = np.lexsort((rows, idx))
    t_ptr = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=I))])
    t_idx, t_val = rows[order], val[order]
    mean = np.bincount(idx, weights=val, minlength=I) / U
    var = np.bincount(idx, weights=val ** 2, minlength=I) / U - mean ** 2
    var = np.where(var.astype(np.float32) < 10 * np.finfo(np.float32).eps, 1.0, var.astype(np.float32).astype(np.float64))
    inv = f32(1.0 / np.sqrt(var))

    def apply(X):
        T = f32(_csr_mm(ptr, idx, val, inv[:, None] * X))
        return f32(inv[:, None] * _csr_mm(t_ptr, t_idx, t_val, T))

    return apply, U, I


def _chol_inv(G):
    try:
        return np.linalg.inv(np.linalg.cholesky(G).T)
    except np.linalg.LinAlgError:
        s, U_ = np.linalg.eigh(G)
        return U_ / np.sqrt(np.maximum(s, s.max() * 1e-14))


def _orth(Y):
    Y = f32(Y @ _chol_inv(Y.T @ Y))
    return f32(Y @ _chol_inv(Y.T @ Y))


def subspace_eigs_restated(apply, n, k, b, tol=1e-5, max_iter=300, seed=2023):
    """(eigenvalues [k], iterations, residuals / lambda_1 [k]); iterations is None when max_iter applications of the
    operator did not reach tol."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    V = _orth(torch.randn(n, b, generator=gen, dtype=torch.float32).numpy().astype(np.float64))
    lam = res = None
    for it in range(1, int(max_iter) + 1):
        W = apply(V)
        VV, VW, WW = V.T @ V, V.T @ W, W.T @ W
        H = 0.5 * (VW + VW.T)
        Li = np.linalg.inv(np.linalg.cholesky(VV))
        lam, Z = np.linalg.eigh(Li @ H @ Li.T)
        order = np.argsort(-lam, kind="stable")
        lam, Q = lam[order], (Li.T @ Z)[:, order]
        r2 = (np.einsum("ij,ik,kj->j", Q, WW, Q) - 2 * lam * np.einsum("ij,ik,kj->j", Q, VW, Q)
              + lam ** 2 * np.einsum("ij,ik,kj->j", Q, VV, Q))
        res = np.sqrt(np.maximum(r2, 0.0))
        if lam[0] > 0 and np.all(res[:k] <= tol * lam[0]):
            return lam[:k].copy(), it, res[:k] / lam[0]
        scale = np.where(lam > 0, 1.0 / np.where(lam > 0, lam, 1.0), 1.0)
        V = _orth(f32(W @ (Q * scale[None, :])))
    return lam[:k].copy(), None, res[:k] / lam[0]
