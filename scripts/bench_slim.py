"""SLIM victim timings (not the driver's bench line): l1_reg = 1, l2_reg = 5, 50 sweeps, on the train edges of
recad_amd.synth.make_device("ml1m") with every value 1.0.  The fit is rk_knn_norms, rk_pca_transpose, rk_ease_gram and
rk_slim_fit; the line gives the whole fit and rk_slim_fit alone on a Gram matrix built beforehand.  Every number is the median of
single calls timed by device events after a warm call.

Counted traffic of the update steps: every coordinate step with delta != 0 reads one row of G, 4 I bytes, and rewrites r inside
LDS; the sum over the columns of info's step counts times 4 I is what the steps moved from L2 / HBM (G itself is 4 I^2 bytes and
stays in the caches at this shape), given over the time of rk_slim_fit.  The chain of steps of a column is sequential: steps /
time / resident workgroups is the rate at which one workgroup takes them.

LDS per workgroup is 8 I + 64 bytes; the workgroups a CU holds is the smaller of 160 KiB over that and the 8 that 32 waves allow.
Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/bench_slim.py --reps 3`, with nothing else traced in it.

    python scripts/bench_slim.py [--shape ml1m] [--l1 1.0] [--l2 5.0] [--sweeps 50] [--reps 9]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU, WAVES_PER_CU, WAVES_PER_WG, N_CU = 160 * 1024, 32, 4, 256


class _Mat:
    def __init__(self, csr, n_users, n_items):
        self.csr, self.n_users, self.n_items = csr, n_users, n_items

    def info_describe(self):
        return {"n_users": self.n_users, "n_items": self.n_items, "train_mat": (*self.csr, self.n_items)}


def _median_ms(fn, reps):
    import torch

    times = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml1m")
    ap.add_argument("--l1", type=float, default=1.0)
    ap.add_argument("--l2", type=float, default=5.0)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    from recad_amd import _lib, model, synth

    dev = torch.device("cuda:0")
    d = synth.make_device(args.shape, dev)
    ptr, idx = d["train"]
    U, I = d["n_users"], d["n_items"]
    rp, idx = ptr.to(torch.int32).contiguous(), idx.to(torch.int32).contiguous()
    nnz = int(idx.numel())
    val = torch.ones(nnz, dtype=torch.float32, device=dev)
    v = model.from_config("victim", "slim", l1_reg=args.l1, l2_reg=args.l2, sweeps=args.sweeps).I(dataset=_Mat((rp, idx, val), U, I)).to(dev)
    v.fit()                                                 # warm: the CSR cache, the kernels' first launches
    torch.cuda.synchronize()
    fit_ms = _median_ms(v.fit, args.reps)
    info = {k: t.cpu().numpy() for k, t in v.fit_info().items()}
    # rk_slim_fit alone, on a Gram matrix of its own
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    colptr = torch.empty(I + 1, dtype=torch.int32, device=dev)
    crow, cval = torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.check(L.rk_pca_transpose(U, I, P(rp), P(idx), P(val), P(colptr), P(crow), P(cval), s), "rk_pca_transpose")
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    G, W = torch.empty(I * I, dtype=torch.float32, device=dev), torch.empty(I * I, dtype=torch.float32, device=dev)
    _lib.check(L.rk_ease_gram(U, I, P(rp), P(idx), P(val), P(colptr), P(crow), P(cval), args.l2, P(G), P(status), s), "rk_ease_gram")

    def solve():
        _lib.check(L.rk_slim_fit(I, P(G), args.l1, args.sweeps, P(W), None, None, P(status), s), "rk_slim_fit")
    solve_ms = _median_ms(solve, args.reps)
    assert torch.equal(W.view(I, I), v.W.data)
    steps = int(info["steps"].astype("int64").sum())
    moved = 4.0 * I * steps
    lds = 8 * I + 64
    wg_per_cu = min(LDS_PER_CU // lds, WAVES_PER_CU // WAVES_PER_WG)
    resident = min(I, wg_per_cu * N_CU)
    print(json.dumps({"shape": args.shape, "n_users": U, "n_items": I, "nnz": nnz, "l1_reg": args.l1, "l2_reg": args.l2, "sweeps": args.sweeps,
                      "reps": args.reps, "fit_ms": round(fit_ms[0], 3), "fit_ms_min_max": [round(fit_ms[1], 3), round(fit_ms[2], 3)],
                      "slim_fit_ms": round(solve_ms[0], 3), "slim_fit_ms_min_max": [round(solve_ms[1], 3), round(solve_ms[2], 3)],
                      "update_steps": steps, "steps_per_column_max": int(info["steps"].max()), "update_row_bytes": moved,
                      "update_tb_per_s_whole_call": round(moved / (solve_ms[0] * 1e-3) / 1e12, 3),
                      "positive_weights": int(info["support"].astype("int64").sum()), "density": round(float(info["support"].sum()) / (I * I), 5),
                      "last_sweep_max": int(info["last_sweep"].max()), "columns_stopped_early": int((info["last_sweep"] < args.sweeps).sum()),
                      "lds_bytes_per_workgroup": lds, "workgroups_per_cu": wg_per_cu, "waves_per_simd": wg_per_cu * WAVES_PER_WG // 4,
                      "resident_workgroups": resident,
                      "us_per_step_of_one_workgroup": round(solve_ms[0] * 1e3 / (steps / resident), 3),
                      "ease_fit_ms_same_shape_for_context": 10.9}))


if __name__ == "__main__":
    main()
