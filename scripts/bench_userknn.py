"""UserKNN victim timings (not the driver's bench line), k = 50 and 100, un-normalised and normalised, on the train edges of
recad_amd.synth.make_device with every value 1.0: the fit as the victim runs it (rk_knn_norms twice, rk_pca_transpose,
rk_itemknn_neighbors on the transposed roles), that neighbour call alone from device inputs prepared once, and one evaluation of
every user with a train list (score_matrix in chunks of 4096 users, so the yelp shape's score matrix is never whole), each by
device events after a warm call.

Beside them, in the same run and process, ItemKNN and RP3beta at the same shape and k: their fits and their score_matrix over the
same chunks.  And the same evaluation composed from torch operations: the kept weights as a sparse U x U matrix (one row block of
4096 users at a time) times the dense U x I rating matrix, torch.sparse.mm; its sums are in no fixed order, so it is a yardstick
for time only.

The scoring kernel's traffic is counted, not sampled: every kept neighbour's row is read once per evaluated user (8 bytes an
entry: column and value), the two tables once, and every score is written once; `gather_share_of_8TBs` is the row bytes alone over
the kernel's time against 8 TB/s, `all_share_of_8TBs` adds tables and output.

Each shape runs in a child process of its own under its own time limit; one JSON line per measurement, appended to --out.

    python scripts/bench_userknn.py [--shapes ml1m,yelp] [--ks 50,100] [--timeout 400] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4096
PEAK_BYTES_PER_S = 8e12


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


def measure(shape, ks, emit):
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
    lens = (rp[1:] - rp[:-1]).long()
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    data = _Mat((rp, idx, val), U, I)
    users = torch.nonzero(lens > 0).view(-1).to(torch.int32).contiguous()
    n = int(users.numel())
    scores = torch.empty(min(n, CHUNK) * I, dtype=torch.float32, device=dev)
    chunks = [users[c:c + CHUNK].contiguous() for c in range(0, n, CHUNK)]

    def evaluation(v):
        def run():
            for c in chunks:
                v.score_matrix(c, scores[: c.numel() * I])
        return run

    # device inputs of the neighbour call, prepared once
    colptr = torch.empty(I + 1, dtype=torch.int32, device=dev)
    crow, cval = torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.check(L.rk_pca_transpose(U, I, P(rp), P(idx), P(val), P(colptr), P(crow), P(cval), s), "rk_pca_transpose")
    rn_user = torch.empty(U, dtype=torch.float32, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.check(L.rk_knn_norms(U, I, P(rp), P(idx), P(val), P(rn_user), P(status), s), "rk_knn_norms")
    dense_bytes = 4 * U * I
    rows_of = torch.repeat_interleave(torch.arange(U, device=dev), lens)
    R_dense = torch.zeros(U, I, dtype=torch.float32, device=dev)
    R_dense[rows_of, idx.long()] = val

    for K in ks:
        base = {"shape": shape, "n_users": U, "n_items": I, "nnz": nnz, "k": K}
        t_id, t_w = torch.empty(K, U, dtype=torch.int32, device=dev), torch.empty(K, U, dtype=torch.float32, device=dev)

        def user_neighbors():
            _lib.check(L.rk_itemknn_neighbors(I, U, P(colptr), P(crow), P(cval), P(rp), P(idx), P(val), P(rn_user), K, 0, None, P(t_id),
                                              P(t_w), s), "rk_itemknn_neighbors")

        victims = [("userknn", model.from_config("victim", "userknn", k=K)),
                   ("userknn_normalized", model.from_config("victim", "userknn", k=K, normalize=True)),
                   ("itemknn", model.from_config("victim", "itemknn", k=K)),
                   ("rp3beta", model.from_config("victim", "rp3beta", k=K))]
        res = {}
        for name, lazy in victims:
            v = lazy.I(dataset=data).to(dev)
            v.fit()                                                           # warm
            torch.cuda.synchronize()
            ids0, w0 = v.nbr_id.clone(), v.nbr_w.data.clone()
            fit_ms = _events(v.fit)
            same = bool(torch.equal(ids0, v.nbr_id) and torch.equal(w0, v.nbr_w.data))
            rec = dict(base, what="fit", victim=name, fit_ms=round(fit_ms, 3), same_bits_every_fit=same)
            if name == "userknn":
                user_neighbors()
                rec["neighbors_kernel_ms"] = round(_events(user_neighbors), 3)
            emit(rec)
            run = evaluation(v)
            run()                                                             # warm
            torch.cuda.synchronize()
            score_ms = _events(run)
            rec = dict(base, what="evaluation", victim=name, n_eval_users=n, chunk=CHUNK, score_matrix_ms=round(score_ms, 3))
            if name.startswith("userknn"):
                kept = v.nbr_id[:, users.long()]                              # [K, n]
                row_bytes = 8.0 * float((lens[kept.clamp(min=0).long()] * (kept >= 0)).sum().item())
                other = 8.0 * K * n + 4.0 * n * I
                rec.update(gathered_row_bytes=row_bytes, mean_kept_neighbours=round(float((kept >= 0).sum().item()) / n, 2),
                           gather_share_of_8TBs=round(row_bytes / (score_ms * 1e-3) / PEAK_BYTES_PER_S, 4),
                           all_share_of_8TBs=round((row_bytes + other) / (score_ms * 1e-3) / PEAK_BYTES_PER_S, 4))
            emit(rec)
            res[name] = (fit_ms, score_ms)
            if name == "userknn":
                # the same evaluation from torch operations: (sparse [block, U]) @ (dense [U, I]) per block of users
                try:
                    blocks = []
                    for c in chunks:
                        sub_id, sub_w = v.nbr_id[:, c.long()], v.nbr_w.data[:, c.long()]
                        keep = sub_id >= 0
                        r = torch.arange(c.numel(), device=dev).expand_as(sub_id)[keep]
                        blocks.append(torch.sparse_coo_tensor(torch.stack([r, sub_id[keep].long()]), sub_w[keep], (c.numel(), U)).coalesce())

                    def composed():
                        for b in blocks:
                            torch.sparse.mm(b, R_dense)

                    composed()                                                # warm
                    torch.cuda.synchronize()
                    torch_ms = _events(composed)
                    v.score_matrix(chunks[0], scores[: chunks[0].numel() * I])
                    ours = scores[: chunks[0].numel() * I].view(-1, I)
                    gap = float((torch.sparse.mm(blocks[0], R_dense) - ours).abs().max().item())
                    emit(dict(base, what="torch_composition", dense_rating_bytes=dense_bytes, score_matrix_ms=round(torch_ms, 3),
                              userknn_over_torch=round(score_ms / torch_ms, 3), max_abs_difference_first_chunk=gap))
                    del blocks
                except Exception as e:                                        # a yardstick that cannot run is reported, not fatal
                    emit(dict(base, what="torch_composition", error=f"{type(e).__name__}: {str(e)[:300]}"))
            del v
        a = res["userknn"]
        emit(dict(base, what="ratio", userknn_over={o: {"fit": round(a[0] / res[o][0], 3), "score_matrix": round(a[1] / res[o][1], 3)}
                                                    for o in ("itemknn", "rp3beta")},
                  normalized_over_plain_score_matrix=round(res["userknn_normalized"][1] / a[1], 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,yelp")
    ap.add_argument("--ks", default="50,100")
    ap.add_argument("--timeout", type=float, default=400.0, help="seconds per shape")
    ap.add_argument("--out", default=None, help="also append every JSON line to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    if a.child:
        measure(a.child, ks, lambda rec: print(json.dumps(rec), flush=True))
        return 0
    rc = 0
    out = open(a.out, "a") if a.out else None
    for shape in a.shapes.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--ks", a.ks], capture_output=True, text=True,
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
