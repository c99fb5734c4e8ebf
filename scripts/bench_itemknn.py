"""ItemKNN victim timings (not the driver's bench line), k = 50, on the train edges of recad_amd.synth.make_device with every
value 1.0: the fit (rk_pca_transpose, rk_knn_norms on the matrix and on its transpose, rk_itemknn_neighbors) and the evaluation
(score_matrix + rk_topk_rows over every user with a train list, K = 100), each by device events after a warm call.

Each quantity stands beside its yardstick, the plain PyTorch way on the same card in the same run:
  fit        a dense fp32 A.T @ A, scaled by the reciprocal column norms, diagonal removed, torch.topk k wide;
  scoring    a dense S from the neighbour tables, A[users] @ S.T (no top-K: the yardstick is the scoring alone, and the HIP
             line reports score_matrix alone as well).
Neither yardstick is bit-exact, and the dense fit breaks ties by torch.topk's order.  The yelp shape reports the fit only: its
dense I x I matrix (4.8 GB fp32) and U x I matrix (7.5 GB) are not what this comparison is about.

Counted work of the fit: adds = sum_u deg(u)^2 integer LDS atomic adds (every pair of items a user rated, both ways, the self
pair included).  No LDS-atomic rate is documented for this part, so no share of peak is given.

Each shape runs in a child process of its own under its own time limit; one JSON line per measurement, appended to --out.

    python scripts/bench_itemknn.py [--shapes ml1m,yelp] [--timeout 400] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, TOPK = 50, 100


def _events(fn, window_s=0.3):
    """ms per call by device events over a window of about window_s (at least 3 calls, at most 500), after one timed probe."""
    import torch

    p0, p1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    p0.record()
    fn()
    p1.record()
    torch.cuda.synchronize()
    reps = int(min(500, max(3, window_s * 1e3 / max(p0.elapsed_time(p1), 1e-3))))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


class _Mat:
    def __init__(self, csr, n_users, n_items):
        self.csr, self.n_users, self.n_items = csr, n_users, n_items

    def info_describe(self):
        return {"n_users": self.n_users, "n_items": self.n_items, "train_mat": (*self.csr, self.n_items)}


def measure(shape, emit):
    sys.path.insert(0, ROOT)
    import torch

    from recad_amd import _lib, model, synth

    dev = torch.device("cuda:0")
    d = synth.make_device(shape, dev)
    ptr, idx = d["train"]
    U, I = d["n_users"], d["n_items"]
    rp, idx = ptr.to(torch.int32).contiguous(), idx.to(torch.int32).contiguous()
    nnz = int(idx.numel())
    val = torch.ones(nnz, dtype=torch.float32, device=dev)
    deg = (rp[1:] - rp[:-1]).double()
    adds = float((deg * deg).sum().item())
    base = {"shape": shape, "n_users": U, "n_items": I, "nnz": nnz, "k": K}
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    v = model.from_config("victim", "itemknn", k=K).I(dataset=_Mat((rp, idx, val), U, I)).to(dev)
    v.fit()                                                               # warm
    torch.cuda.synchronize()
    ids0, w0 = v.nbr_id.clone(), v.nbr_w.data.clone()
    fit_ms = _events(v.fit)
    same = bool(torch.equal(ids0, v.nbr_id) and torch.equal(w0, v.nbr_w.data))
    # the neighbour kernel alone
    colptr = torch.empty(I + 1, dtype=torch.int32, device=dev)
    crow, cval = torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.check(L.rk_pca_transpose(U, I, P(rp), P(idx), P(val), P(colptr), P(crow), P(cval), s), "rk_pca_transpose")
    rn = torch.empty(I, dtype=torch.float32, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.check(L.rk_knn_norms(I, U, P(colptr), P(crow), P(cval), P(rn), P(status), s), "rk_knn_norms")
    t_id, t_w = torch.empty(K, I, dtype=torch.int32, device=dev), torch.empty(K, I, dtype=torch.float32, device=dev)

    def nbr():
        _lib.check(L.rk_itemknn_neighbors(U, I, P(rp), P(idx), P(val), P(colptr), P(crow), P(cval), P(rn), K, 0, None, P(t_id), P(t_w), s),
                   "rk_itemknn_neighbors")
    nbr()
    kernel_ms = _events(nbr)
    emit(dict(base, what="fit", path="hip", fit_ms=round(fit_ms, 3), neighbors_kernel_ms=round(kernel_ms, 3), lds_adds=adds,
              lds_adds_per_s=round(adds / (kernel_ms * 1e-3), 0), same_bits_every_fit=same))
    if shape != "ml1m":
        return
    rows = torch.repeat_interleave(torch.arange(U, device=dev), (rp[1:] - rp[:-1]).long())

    def dense_fit():
        A = torch.zeros(U, I, dtype=torch.float32, device=dev)
        A[rows, idx.long()] = val
        D = A.T @ A
        r = torch.rsqrt(D.diagonal().clamp_min(1e-30))
        W = (D * r[:, None]) * r[None, :]
        W.fill_diagonal_(0)
        return torch.topk(W, K, dim=1)
    ref = dense_fit()                                                     # warm
    torch.cuda.synchronize()
    dense_ms = _events(dense_fit, 1.0)
    err = float((ref.values.t() - w0).abs().max().item())
    emit(dict(base, what="fit", path="torch-dense", dense_ms=round(dense_ms, 3), max_abs_weight_diff_to_hip=err, dense_bytes=4 * I * I + 4 * U * I))
    # evaluation: every user with a train list
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
    evaluate()                                                            # warm
    torch.cuda.synchronize()
    score_ms, eval_ms = _events(score), _events(evaluate)
    emit(dict(base, what="evaluation", path="hip", n_eval_users=n, score_matrix_ms=round(score_ms, 3), score_and_topk_ms=round(eval_ms, 3),
              table_reads=K * I * ((n + 15) // 16)))
    S = torch.zeros(I, I, dtype=torch.float32, device=dev)
    ok = ids0 >= 0
    item = torch.arange(I, device=dev).expand(K, I)
    S[item[ok], ids0[ok].long()] = w0[ok]
    A = torch.zeros(U, I, dtype=torch.float32, device=dev)
    A[rows, idx.long()] = val

    def dense_score():
        return A[users.long()] @ S.T
    ref = dense_score()                                                   # warm
    torch.cuda.synchronize()
    dense_ms = _events(dense_score, 1.0)
    err = float((ref - scores.view(n, I)).abs().max().item())
    emit(dict(base, what="evaluation", path="torch-dense", n_eval_users=n, dense_score_ms=round(dense_ms, 3), max_abs_diff_to_hip=err,
              dense_bytes=4 * I * I + 4 * U * I))


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
