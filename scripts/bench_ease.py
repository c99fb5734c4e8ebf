"""EASE victim timings (not the driver's bench line), lambda = 500, on the train edges of recad_amd.synth.make_device with every
value 1.0: the fit (rk_knn_norms, rk_pca_transpose, rk_ease_gram, rk_ease_invert, rk_ease_weights), its stages one by one, and the
evaluation (score_matrix + rk_topk_rows over every user with a train list, K = 100).  Every number is the median of single calls
timed by device events after a warm call.

The outside yardstick is torch.linalg.inv on the same fp32 matrix on the same card in the same run (a vendor solver: LU with
pivoting, its own workspace).  Both inverses are compared with each other and by the residual max|A P - I|.

Counted work of the inverse: 2 I^3 flops (every block step subtracts a rank-b product from the whole matrix: 2 I^2 b flops, I / b
steps; the panels and the pivot blocks add 4 I b^2 + 2 b^3 per step and are not counted).  The line gives that count over the
WHOLE rk_ease_invert call as a share of the 157.3 TF fp32 MFMA peak: a lower bound of the trailing kernel's own share, since the
call also holds the pivot and panel kernels and the gaps between launches.  Each step reads and writes the matrix once, 8 I^2
bytes, so the call moves 8 I^3 / b bytes: the line gives that over the call's time as well.

The yelp shape (34 474 items, a 4.75 GB matrix) reports the fit and its stages only.

Each shape runs in a child process of its own under its own time limit; one JSON line per measurement, appended to --out.

    python scripts/bench_ease.py [--shapes ml1m,yelp] [--timeout 400] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM, TOPK, PEAK_F32_MFMA_TF = 500.0, 100, 157.3


def _median_ms(fn, reps, before=None):
    """Median over `reps` single calls of fn, each between two device events, after one warm call; `before` runs untimed ahead
    of every call."""
    import torch

    times = []
    for r in range(reps + 1):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


class _Mat:
    def __init__(self, csr, n_users, n_items):
        self.csr, self.n_users, self.n_items = csr, n_users, n_items

    def info_describe(self):
        return {"n_users": self.n_users, "n_items": self.n_items, "train_mat": (*self.csr, self.n_items)}


def measure(shape, emit):
    sys.path.insert(0, ROOT)
    import torch

    from recad_amd import _lib, model, synth
    from recad_amd.victim.ease import resolved_block

    dev = torch.device("cuda:0")
    d = synth.make_device(shape, dev)
    ptr, idx = d["train"]
    U, I = d["n_users"], d["n_items"]
    rp, idx = ptr.to(torch.int32).contiguous(), idx.to(torch.int32).contiguous()
    nnz = int(idx.numel())
    val = torch.ones(nnz, dtype=torch.float32, device=dev)
    big = shape != "ml1m"
    reps = 3 if big else 9
    base = {"shape": shape, "n_users": U, "n_items": I, "nnz": nnz, "reg_lambda": LAM, "reps": reps}
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    v = model.from_config("victim", "ease", reg_lambda=LAM).I(dataset=_Mat((rp, idx, val), U, I)).to(dev)
    v.fit()
    torch.cuda.synchronize()
    fit_ms = _median_ms(v.fit, reps)
    # the stages on buffers of their own
    b = resolved_block(I, None)
    colptr = torch.empty(I + 1, dtype=torch.int32, device=dev)
    crow, cval = torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.check(L.rk_pca_transpose(U, I, P(rp), P(idx), P(val), P(colptr), P(crow), P(cval), s), "rk_pca_transpose")
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    A = v.B.data                                                           # reuse the model's storage: no second I x I beside A0
    A0 = torch.empty_like(A)
    work = torch.empty(I * b, dtype=torch.float32, device=dev)

    def gram():
        _lib.check(L.rk_ease_gram(U, I, P(rp), P(idx), P(val), P(colptr), P(crow), P(cval), LAM, P(A), P(status), s), "rk_ease_gram")

    def invert():
        _lib.check(L.rk_ease_invert(I, P(A), P(work), work.numel(), 0, P(status), s), "rk_ease_invert")

    def weights():
        _lib.check(L.rk_ease_weights(I, P(A), P(A), s), "rk_ease_weights")

    gram_ms = _median_ms(gram, reps)
    A0.copy_(A)
    invert_ms = _median_ms(invert, reps, before=lambda: A.copy_(A0))
    P_hip = A.clone() if not big else None
    weights_ms = _median_ms(weights, reps, before=lambda: A.copy_(A0))
    flops, moved = 2.0 * I ** 3, 8.0 * I ** 3 / b
    tf = flops / (invert_ms[0] * 1e-3) / 1e12
    emit(dict(base, what="fit", path="hip", block=b, fit_ms=round(fit_ms[0], 3), fit_ms_min_max=[round(fit_ms[1], 3), round(fit_ms[2], 3)],
              gram_ms=round(gram_ms[0], 3), invert_ms=round(invert_ms[0], 3), invert_ms_min_max=[round(invert_ms[1], 3), round(invert_ms[2], 3)],
              weights_ms=round(weights_ms[0], 3), invert_flops=flops, invert_tflops_whole_call=round(tf, 2),
              invert_share_of_f32_mfma_peak_whole_call=round(tf / PEAK_F32_MFMA_TF, 4), invert_bytes=moved,
              invert_tb_per_s_whole_call=round(moved / (invert_ms[0] * 1e-3) / 1e12, 3)))
    if big:
        return
    # the yardstick: torch.linalg.inv of the same matrix
    out = torch.empty_like(A0)

    def torch_inv():
        torch.linalg.inv(A0, out=out)
    inv_ms = _median_ms(torch_inv, reps)
    eye = torch.eye(I, device=dev, dtype=torch.float64)
    A64 = A0.double()
    res_hip = float((A64 @ P_hip.double() - eye).abs().max().item())
    res_torch = float((A64 @ out.double() - eye).abs().max().item())
    emit(dict(base, what="inverse", path="torch.linalg.inv", inv_ms=round(inv_ms[0], 3), inv_ms_min_max=[round(inv_ms[1], 3), round(inv_ms[2], 3)],
              max_abs_diff_to_hip=float((out - P_hip).abs().max().item()), max_abs_P=float(out.abs().max().item()),
              residual_hip=res_hip, residual_torch=res_torch))
    del eye, A64, out, P_hip
    # evaluation: every user with a train list
    v.fit()
    users = torch.nonzero(rp[1:] > rp[:-1]).view(-1).to(torch.int32).contiguous()
    n = int(users.numel())
    scores = torch.empty(n * I, dtype=torch.float32, device=dev)
    top_ids, top_scores = torch.empty(n, TOPK, dtype=torch.int32, device=dev), torch.empty(n, TOPK, dtype=torch.float32, device=dev)
    tg = torch.zeros(1, dtype=torch.int32, device=dev)
    tscore, trank = torch.empty(n, 1, dtype=torch.float32, device=dev), torch.empty(n, 1, dtype=torch.int32, device=dev)

    def score():
        v.score_matrix(users, scores)

    def evaluate():
        v.score_matrix(users, scores)
        _lib.check(L.rk_topk_rows(P(scores), n, I, P(users), P(rp), P(idx), TOPK, P(top_ids), P(top_scores), P(tg), 1, P(tscore), P(trank), s),
                   "rk_topk_rows")
    score_ms, eval_ms = _median_ms(score, reps), _median_ms(evaluate, reps)
    X = torch.zeros(U, I, dtype=torch.float32, device=dev)
    X[torch.repeat_interleave(torch.arange(U, device=dev), (rp[1:] - rp[:-1]).long()), idx.long()] = val
    Bm = v.B.data

    def dense_score():
        return X[users.long()] @ Bm
    dense_ms = _median_ms(dense_score, reps)
    err = float((dense_score() - scores.view(n, I)).abs().max().item())
    emit(dict(base, what="evaluation", path="hip", n_eval_users=n, score_matrix_ms=round(score_ms[0], 3), score_and_topk_ms=round(eval_ms[0], 3),
              b_row_reads_bytes=4.0 * nnz * I, torch_dense_score_ms=round(dense_ms[0], 3), max_abs_diff_to_torch_dense=err))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,yelp")
    ap.add_argument("--timeout", type=float, default=400.0, help="seconds per shape")
    ap.add_argument("--out", default=None, help="also append every JSON line to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        measure(a.child, lambda rec: print(json.dumps(rec), flush=True))
        return 0
    rc = 0
    out = open(a.out, "a") if a.out else None
    for shape in a.shapes.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape], capture_output=True, text=True,
                               timeout=a.timeout, cwd=ROOT)
            lines, err = p.stdout, (None if p.returncode == 0 else f"exit {p.returncode}: {p.stderr[-1500:]}")
        except subprocess.TimeoutExpired as e:
            lines, err = (e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")), f"time limit {a.timeout:.0f} s"
        for line in lines.strip().splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
        if err:
            print(json.dumps({"shape": shape, "error": err}), flush=True)
            rc = 1
            break                   # a failed GPU child ends the run: nothing more is started on the card
    if out:
        out.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
