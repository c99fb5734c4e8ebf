"""Randomised check of the LDS-resident sliced SpMM (rk_spmm_lds) in a random FORM (slice widths of the two tables, chunk cap:
rk_lds_plan_build_host_ex) against the numpy walk of its own plan (tests/_lds_restate.py):
    python tests/tools/spmm_lds_stress.py <seed> <n_cases>
Random bipartite graphs (tiny classes, empty rows, rows longer than every chunk cap, dense and sparse), every dim that is a
multiple of 4 up to 256, plan -> pack -> rk_spmm_lds -> unpack.  Up to 200 000 stored entries the result is held to the walk's
contracts: without an addend the walk's bits; with one, two roundings of the exact (acc * dinv + add).  Larger cases keep the
comparison with the oracle's CSR product.  The forms are tried in a random order (one may not divide dim or fit the LDS); a graph none fits gets the planner's choice."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import oracle as orc  # noqa: E402
from recad_amd import _lib  # noqa: E402
from recad_amd.graph import CsrGraph  # noqa: E402
from tests import _lds_restate as R  # noqa: E402

WALK_NNZ = 200_000


def make_case(rng):
    U = int(rng.choice([1, 3, 17, 64, 300, 1500, 5000, 9000]))
    I = int(rng.choice([1, 2, 16, 33, 200, 1200, 3700, 9000]))
    d = int(rng.choice([4, 8, 12, 32, 48, 64, 100, 128, 256]))
    dens = float(rng.choice([0.002, 0.02, 0.2, 0.9]))
    deg = rng.binomial(I, dens, U)
    if rng.random() < 0.5:
        deg[rng.integers(0, U)] = I            # one full row
    if rng.random() < 0.5:
        deg[rng.integers(0, U, max(1, U // 10))] = 0   # empty rows
    if deg.sum() == 0:
        deg[0] = min(I, 1)
    ptr = np.zeros(U + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(deg)
    idx = np.concatenate([np.sort(rng.choice(I, size=int(k), replace=False)) for k in deg]).astype(np.int32) if deg.sum() else np.zeros(0, np.int32)
    forms = [list(R.FORMS)[k] for k in rng.permutation(len(R.FORMS))]   # tried in this order: the first that fits the graph and divides dim
    cap = int(rng.choice([0, 64, 96, 128, 256, 512]))
    n_cu = int(rng.choice([2, 8, 64, 256]))
    return U, I, d, dens, ptr, idx, forms, cap, n_cu


def run(seed=0, n_cases=50, device=None, verbose=False):
    """-> the set of (lpa, lpb) forms that ran"""
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda:0") if device is None else device
    worst, done, skipped, walked, forms = 0.0, 0, 0, 0, set()
    L = _lib.lib()
    for case in range(n_cases):
        U, I, d, dens, ptr, idx, try_forms, cap, n_cu = make_case(rng)
        rowptr, col, val = R.norm_adj_csr(U, I, ptr, idx)
        plan = None
        for form in try_forms:
            plan, info, rc, n_words = R.build_plan_handle(U, I, rowptr, col, val, d, n_cu, R.FORMS[form], cap)
            assert rc == 0, L.rk_last_error()
            if plan is not None:
                break
        if plan is None:
            plan, info, rc, n_words = R.build_plan_handle(U, I, rowptr, col, val, d, n_cu)
        if plan is None:
            skipped += 1
            continue
        try:
            words = R.plan_words(plan, n_words)
            buf = torch.zeros(n_words + 4, device=dev, dtype=torch.int32)
            buf = buf[((-buf.data_ptr() // 4) % 4):][:n_words]
            _lib.check(L.rk_lds_plan_upload(plan, _lib.ptr(buf), _lib.stream_ptr()), "rk_lds_plan_upload")
        finally:
            L.rk_lds_plan_destroy(plan)
        g = CsrGraph.from_user_item_csr(U, I, ptr, idx, dev)
        g.__dict__.setdefault("_lds", {})[d] = (buf, info)
        forms.add((info.lpa, info.lpb))
        N = U + I
        x = rng.standard_normal((N, d), dtype=np.float32)
        add = rng.standard_normal((N, d), dtype=np.float32)
        xt, at = torch.from_numpy(x).to(dev), torch.from_numpy(add).to(dev)
        y = g.spmm_lds(xt, at).cpu().numpy()
        y2 = g.spmm_lds(xt, at).cpu().numpy()
        y0 = g.spmm_lds(xt).cpu().numpy()
        tag = (case, U, I, d, dens, (info.lpa, info.lpb), hex(info.chunk), n_cu)
        assert np.array_equal(y, y2) and np.array_equal(y0, g.spmm_lds(xt).cpu().numpy()), (tag, "not reproducible")
        if len(col) <= WALK_NNZ:
            w = R.walk(words, x, check_banks=False)
            assert w.entries == len(col), tag
            assert np.array_equal(y0, w.y0), (tag, "differs from the walk", int((y0 != w.y0).sum()))
            exact, bud = R.addend_budget(w, add)
            assert (np.abs(y - exact) <= bud).all(), (tag, "addend beyond two roundings")
            walked += 1
        ref = orc.spmm(rowptr, col, val, x)
        err = float(np.abs(y - (ref + add)).max() / max(np.abs(ref + add).max(), 1e-30))
        assert err < 3e-6, (tag, err)
        worst = max(worst, err)
        done += 1
        if verbose:
            print(tag, f"{err:.2e}")
    print(f"seed {seed}: {done} cases clean ({walked} against the walk bit for bit, {skipped} graphs did not qualify), forms {sorted(forms)}, "
          f"worst relative error against the oracle {worst:.2e}")
    return forms


if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 0, int(sys.argv[2]) if len(sys.argv) > 2 else 50, verbose=True)
