"""RP3beta victim timings (not the driver's bench line), the defaults (alpha = 1, beta = 0.6, k = 100), on the train edges of
recad_amd.synth.make_device with every value 1.0: the fit as the victim runs it and by entry point (rk_rp3_steps, rk_rp3_factors,
rk_rp3_neighbors, each from device inputs prepared once), and one evaluation of every user with a train list (score_matrix in
chunks of 4096 users, so the yelp shape's 7.5 GB score matrix is never whole), each by device events after a warm call.

Beside them, in the same run and process, the yardstick: ItemKNN at the same shape and k -- its fit, its neighbour kernel and its
score_matrix over the same chunks.  Both fits add sum_u deg(u)^2 numbers in LDS (every pair of items a user rated, both ways, the
self pair included): ItemKNN 32-bit integers, RP3beta 64-bit ones, over half the band.  No LDS-atomic rate is documented for this
part, so no share of peak is given; the adds per second of both are reported.

Each shape runs in a child process of its own under its own time limit; one JSON line per measurement, appended to --out.

    python scripts/bench_rp3beta.py [--shapes ml1m,yelp] [--timeout 400] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4096


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

    from recad_amd import _lib, default, model, synth

    dev = torch.device("cuda:0")
    d = synth.make_device(shape, dev)
    ptr, idx = d["train"]
    U, I = d["n_users"], d["n_items"]
    rp, idx = ptr.to(torch.int32).contiguous(), idx.to(torch.int32).contiguous()
    nnz = int(idx.numel())
    val = torch.ones(nnz, dtype=torch.float32, device=dev)
    deg = (rp[1:] - rp[:-1]).double()
    adds = float((deg * deg).sum().item())
    cfg = default.MODEL["victim"]["rp3beta"]
    alpha, beta, K = float(cfg["alpha"]), float(cfg["beta"]), int(cfg["k"])
    base = {"shape": shape, "n_users": U, "n_items": I, "nnz": nnz, "k": K}
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    data = _Mat((rp, idx, val), U, I)
    rp3 = model.from_config("victim", "rp3beta").I(dataset=data).to(dev)
    knn = model.from_config("victim", "itemknn", k=K).I(dataset=data).to(dev)
    users = torch.nonzero(rp[1:] > rp[:-1]).view(-1).to(torch.int32).contiguous()
    n = int(users.numel())
    scores = torch.empty(min(n, CHUNK) * I, dtype=torch.float32, device=dev)
    chunks = [users[c:c + CHUNK].contiguous() for c in range(0, n, CHUNK)]

    def evaluation(v):
        def run():
            for c in chunks:
                v.score_matrix(c, scores[: c.numel() * I])
        return run

    # device inputs of the entry points, prepared once
    colptr = torch.empty(I + 1, dtype=torch.int32, device=dev)
    crow, cval = torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.check(L.rk_pca_transpose(U, I, P(rp), P(idx), P(val), P(colptr), P(crow), P(cval), s), "rk_pca_transpose")
    rn = torch.empty(I, dtype=torch.float32, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.check(L.rk_knn_norms(I, U, P(colptr), P(crow), P(cval), P(rn), P(status), s), "rk_knn_norms")
    steps, r = torch.empty(nnz, dtype=torch.int64, device=dev), torch.empty(U, dtype=torch.int64, device=dev)
    fa, fb = torch.empty(I, dtype=torch.float64, device=dev), torch.empty(I, dtype=torch.float64, device=dev)
    t_id, t_w = torch.empty(K, I, dtype=torch.int32, device=dev), torch.empty(K, I, dtype=torch.float32, device=dev)

    def rp3_steps():
        _lib.check(L.rk_rp3_steps(U, P(rp), P(val), alpha, P(steps), P(r), s), "rk_rp3_steps")

    def rp3_factors():
        _lib.check(L.rk_rp3_factors(I, P(colptr), alpha, beta, P(fa), P(fb), s), "rk_rp3_factors")

    def rp3_neighbors():
        _lib.check(L.rk_rp3_neighbors(U, I, P(rp), P(idx), P(steps), P(colptr), P(crow), P(fa), P(fb), K, 0, None, P(t_id), P(t_w), s),
                   "rk_rp3_neighbors")

    def knn_neighbors():
        _lib.check(L.rk_itemknn_neighbors(U, I, P(rp), P(idx), P(val), P(colptr), P(crow), P(cval), P(rn), K, 0, None, P(t_id), P(t_w), s),
                   "rk_itemknn_neighbors")

    res = {}
    for name, v, nbr in (("rp3beta", rp3, rp3_neighbors), ("itemknn", knn, knn_neighbors)):
        v.fit()                                                           # warm
        torch.cuda.synchronize()
        ids0, w0 = v.nbr_id.clone(), v.nbr_w.data.clone()
        fit_ms = _events(v.fit)
        same = bool(torch.equal(ids0, v.nbr_id) and torch.equal(w0, v.nbr_w.data))
        rec = dict(base, what="fit", victim=name, fit_ms=round(fit_ms, 3), same_bits_every_fit=same)
        if name == "rp3beta":
            for fn in (rp3_steps, rp3_factors):
                fn()                                                      # warm, and the neighbour entry's inputs
            rec.update(steps_ms=round(_events(rp3_steps), 4), factors_ms=round(_events(rp3_factors), 4))
        nbr()
        kernel_ms = _events(nbr)
        rec.update(neighbors_kernel_ms=round(kernel_ms, 3), lds_adds=adds, lds_add_bytes=8 if name == "rp3beta" else 4,
                   lds_adds_per_s=round(adds / (kernel_ms * 1e-3), 0))
        emit(rec)
        run = evaluation(v)
        run()                                                             # warm
        torch.cuda.synchronize()
        score_ms = _events(run)
        emit(dict(base, what="evaluation", victim=name, n_eval_users=n, chunk=CHUNK, score_matrix_ms=round(score_ms, 3)))
        res[name] = (fit_ms, kernel_ms, score_ms)
    a, b = res["rp3beta"], res["itemknn"]
    emit(dict(base, what="ratio", rp3beta_over_itemknn={"fit": round(a[0] / b[0], 3), "neighbors_kernel": round(a[1] / b[1], 3),
                                                        "score_matrix": round(a[2] / b[2], 3)}))


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
