"""CatchSyncSelectUsers defender timings (not the driver's bench line): for each synthetic shape (ml1m, yelp: the train edges of
recad_amd.synth.make_device, every value 1.0) the device-event time of rk_cs_user_sums for form wave / workgroup / automatic
and schedule work / natural, the device-event time of the other entries (rk_cs_features, rk_cs_cells, rk_cs_scores), and the
wall time of one whole defense_step (norms, transpose, features, cells, order, sums, scores, selection; a host clock around
work that ends in a device synchronise).  Each timing is repeated three times in the run; the lines carry the three values.

Counted work of rk_cs_user_sums: bytes = 4 nnz + 16 U (every column id once, two int64 per user; the cell tables stay in
cache), lds_atomics = nnz.  GBs = bytes over the kernel time: a rate of the algorithm's traffic, not a share of peak.

The comparator is the same integers composed from torch ops on the same card in the same run (bincount, index_add_, unique on
the item keys and on the (user, cell) pairs), timed the same way AFTER its pair_num / back_num / cell table have been checked
equal to the HIP path's.  "torch_sums" covers what rk_cs_user_sums covers, "torch_all" the features, cells, sums and scores.

Each shape runs in a child process of its own under its own time limit; one JSON line per measurement, appended to --out.

    python scripts/bench_cs_defender.py [--shapes ml1m,yelp] [--timeout 400] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS, MIN_ITEMS = 1, 20


def _events(fn, window_s=0.5):
    """ms per call by device events over a window of about window_s (at least 10 calls, at most 2000), after one timed probe."""
    import torch

    p0, p1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    p0.record()
    fn()
    p1.record()
    torch.cuda.synchronize()
    reps = int(min(2000, max(10, window_s * 1e3 / max(p0.elapsed_time(p1), 1e-3))))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _three(fn):
    return [round(_events(fn), 4) for _ in range(3)]


def _bucket(x, s):
    """bucket(x, s) of include/recad_hip.h on an int64 tensor of values >= 1: shifts and masks only."""
    import torch

    e = torch.zeros_like(x)
    for k in range(1, 32):
        e += (x >> k) > 0
    return e * (1 << s) + (((x << s) >> e) & ((1 << s) - 1))


def torch_features_cells(rp, col, U, I):
    import torch

    d = (rp[1:] - rp[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(U, device=col.device), d)
    c64 = col.long()
    deg = torch.bincount(c64, minlength=I)
    reach = torch.zeros(I, dtype=torch.int64, device=col.device).index_add_(0, c64, d[rows])
    rated = deg > 0
    key = _bucket(deg.clamp_min(1), BITS) * 65536 + _bucket(reach.clamp_min(1), BITS)
    uniq, inv, counts = torch.unique(key[rated], return_inverse=True, return_counts=True)
    cell_of = torch.full((I,), -1, dtype=torch.int64, device=col.device)
    cell_of[rated] = inv
    return d, rows, cell_of, counts


def torch_sums(rows, col, cell_of, counts, U):
    import torch

    M = counts.numel()
    c = cell_of[col.long()]
    back = torch.zeros(U, dtype=torch.int64, device=col.device).index_add_(0, rows, counts[c])
    pairs, n_uc = torch.unique(rows * M + c, return_counts=True)
    pair = torch.zeros(U, dtype=torch.int64, device=col.device).index_add_(0, torch.div(pairs, M, rounding_mode="floor"), n_uc * n_uc)
    return pair, back


def torch_sync(d, pair):
    import torch

    dd = d.double()
    return torch.where(d >= MIN_ITEMS, (pair.double() - dd) / (dd * (dd - 1.0)), torch.full_like(dd, -1.0)).float()


def measure(shape, emit):
    sys.path.insert(0, ROOT)
    import torch

    from recad_amd import _lib, model, synth
    from recad_amd.defense.catchsync_select_users import work_order

    dev = torch.device("cuda:0")
    data = synth.make_device(shape, dev)
    ptr, idx = data["train"]
    U, I = data["n_users"], data["n_items"]
    rp, col = ptr.to(torch.int32).contiguous(), idx.to(torch.int32).contiguous()
    nnz = int(col.numel())
    val = torch.ones(nnz, dtype=torch.float32, device=dev)
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    colptr = torch.empty(I + 1, dtype=torch.int32, device=dev)
    crow, cval = torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.check(L.rk_pca_transpose(U, I, P(rp), P(col), P(val), P(colptr), P(crow), P(cval), s), "rk_pca_transpose")
    deg, reach = torch.empty(I, dtype=torch.int32, device=dev), torch.empty(I, dtype=torch.int32, device=dev)
    cell_of, cell_count = torch.empty(I, dtype=torch.int32, device=dev), torch.empty(_lib.RK_CS_MAX_CELLS, dtype=torch.int32, device=dev)
    info, status = torch.empty(4, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    pair, back = torch.empty(U, dtype=torch.int64, device=dev), torch.empty(U, dtype=torch.int64, device=dev)
    score = torch.empty(U, dtype=torch.float32, device=dev)

    def features():
        _lib.check(L.rk_cs_features(U, I, P(rp), P(colptr), P(crow), P(deg), P(reach), s), "rk_cs_features")

    def cells():
        _lib.check(L.rk_cs_cells(I, P(deg), P(reach), BITS, P(cell_of), P(cell_count), P(info), P(status), s), "rk_cs_cells")

    features()
    cells()
    M = int(info[0].item())
    order = work_order(rp)
    d_len = (rp[1:] - rp[:-1])
    base = {"shape": shape, "n_users": U, "n_items": I, "nnz": nnz, "grid_bits": BITS, "n_cells": M, "longest_row": int(d_len.max().item()),
            "sums_bytes": 4 * nnz + 16 * U}

    def scores():
        _lib.check(L.rk_cs_scores(U, P(rp), P(pair), P(back), P(info), 0, MIN_ITEMS, P(score), s), "rk_cs_scores")

    # the comparator's integers first: equal or nothing is timed
    t_d, t_rows, t_cell, t_counts = torch_features_cells(rp, col, U, I)
    t_pair, t_back = torch_sums(t_rows, col, t_cell, t_counts, U)
    first = None
    for form, fname in ((1, "wave"), (2, "workgroup"), (0, "auto")):
        for schedule in ("work", "natural"):
            def sums():
                _lib.check(L.rk_cs_user_sums(U, P(rp), P(col), P(cell_of), P(cell_count), M, form, P(order) if schedule == "work" else None,
                                             P(pair), P(back), s), "rk_cs_user_sums")
            pair.fill_(-1)
            back.fill_(-1)
            sums()
            torch.cuda.synchronize()
            if first is None:
                first = (pair.clone(), back.clone())
                equal = bool(torch.equal(pair, t_pair) and torch.equal(back, t_back) and torch.equal(cell_of.long(), t_cell)
                             and torch.equal(cell_count[:M].long(), t_counts))
                if not equal:
                    raise SystemExit("the torch comparator and the HIP path disagree on the integers")
            same = bool(torch.equal(first[0], pair) and torch.equal(first[1], back))
            ms = _three(sums)
            dfd = model.from_config("defender", "CatchSyncSelectUsers", attack_num=50, schedule=schedule,
                                    form=None if form == 0 else fname, device=dev).I(dataset=(rp, col, val, I))
            dfd.defense_step()                                            # warm
            torch.cuda.synchronize()
            n_steps = 50 if shape == "ml1m" else 10
            step_ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                for _ in range(n_steps):
                    dfd.defense_step()
                torch.cuda.synchronize()
                step_ms.append(round((time.perf_counter() - t0) / n_steps * 1e3, 3))
            emit(dict(base, path="hip", form=fname, schedule=schedule, user_sums_ms=ms, defense_step_ms=step_ms,
                      sums_GBs=round(base["sums_bytes"] / (min(ms) * 1e-3) / 1e9, 1), same_words_as_first=same, equals_torch=True))
    scores()
    torch.cuda.synchronize()
    t_score = torch_sync(t_d, t_pair)
    emit(dict(base, path="hip", features_ms=_three(features), cells_ms=_three(cells), scores_ms=_three(scores),
              scores_equal_torch_bits=bool(torch.equal(score.view(torch.int32), t_score.view(torch.int32)))))

    def torch_all():
        d, rows, c, n = torch_features_cells(rp, col, U, I)
        p, _ = torch_sums(rows, col, c, n, U)
        return torch_sync(d, p)

    torch_all()
    torch.cuda.synchronize()
    emit(dict(base, path="torch", torch_sums_ms=_three(lambda: torch_sums(t_rows, col, t_cell, t_counts, U)), torch_all_ms=_three(torch_all)))


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
