"""FraudarSelectUsers defender timings (not the driver's bench line): for each synthetic shape (tiny, ml1m, yelp: the train
edges of recad_amd.synth.make_device, every value 1.0, log weights at offset 5) the device-event time of rk_fd_init, of the whole
peel (rk_fd_peel_ex) at the library's steps_per_launch and at its two neighbours, the same per step, and the wall time of one
whole defense_step (norms, transpose, table, init, peel, block; a host clock around work that ends in a device synchronise).
Each timing is repeated three times in the run; the lines carry the three values.  pri is destroyed by a peel, so rk_fd_init runs
again before every timed peel, outside the events.

The peel is one workgroup walking a chain of N dependent steps: its time is latency, not traffic, so no rate is derived.  What
the steps did is counted from the result instead: how many of the t* steps before the best block removed users, and how many
edges were charged from a user step against an item step (every edge is charged once, from whichever end goes first).

For orientation only, not a baseline to beat: the wall time of the Python heap restatement (tests/_fraudar_restate.py) on the
same input; its order, step_of and best block are compared with the device's words before anything is reported.

Each shape runs in a child process of its own under its own time limit; one JSON line per measurement, appended to --out.

    python scripts/bench_fraudar.py [--shapes tiny,ml1m,yelp] [--timeout 500] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(shape, emit):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from recad_amd import _lib, model, synth
    from recad_amd.defense.fraudar_select_users import weight_table
    from tests import _fraudar_restate as R

    dev = torch.device("cuda:0")
    data = synth.make_device(shape, dev)
    ptr, idx = data["train"]
    U, I = data["n_users"], data["n_items"]
    N = U + I
    rp, col = ptr.to(torch.int32).contiguous(), idx.to(torch.int32).contiguous()
    nnz = int(col.numel())
    val = torch.ones(nnz, dtype=torch.float32, device=dev)
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    colptr = torch.empty(I + 1, dtype=torch.int32, device=dev)
    crow, cval = torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.check(L.rk_pca_transpose(U, I, P(rp), P(col), P(val), P(colptr), P(crow), P(cval), s), "rk_pca_transpose")
    wtab = torch.from_numpy(weight_table(U, "log", 5.0).view(np.int32)).to(dev)
    w_item = torch.empty(I, dtype=torch.int32, device=dev)
    pri = torch.empty(N, dtype=torch.int64, device=dev)
    info, status = torch.empty(4, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    order, step_of = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)

    def init():
        _lib.check(L.rk_fd_init(U, I, nnz, P(rp), P(col), P(colptr), P(wtab), P(w_item), P(pri), P(info), P(status), s), "rk_fd_init")

    def peel(spl):
        _lib.check(L.rk_fd_peel_ex(U, I, nnz, P(rp), P(col), P(colptr), P(crow), P(w_item), P(pri), P(order), P(step_of), None, P(info),
                                   spl, s), "rk_fd_peel_ex")

    def timed(fn, before=None):
        out = []
        for _ in range(3):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(round(e0.elapsed_time(e1), 4))
        return out

    base = {"shape": shape, "n_users": U, "n_items": I, "n_nodes": N, "nnz": nnz,
            "longest_row": int((rp[1:] - rp[:-1]).max().item()), "longest_column": int((colptr[1:] - colptr[:-1]).max().item())}
    default = _lib.RK_FD_STEPS_PER_LAUNCH
    init()
    peel(default)                                                   # warm; also the words every other setting must repeat
    torch.cuda.synchronize()
    first = (order.clone(), step_of.clone(), info.clone())
    emit(dict(base, entry="rk_fd_init", ms=timed(init)))
    for spl in (default // 4, default, default * 4):
        ms = timed(lambda: peel(spl), before=init)
        same = bool(torch.equal(first[0], order) and torch.equal(first[1], step_of) and torch.equal(first[2], info))
        emit(dict(base, entry="rk_fd_peel_ex", steps_per_launch=spl, launches=-(-N // spl), ms=ms, us_per_step=round(min(ms) * 1e3 / N, 3),
                  same_words_as_default=same))
    t_best, f_best, n_best, f_0 = first[2].cpu().tolist()
    so = first[1].long()
    rows = torch.repeat_interleave(torch.arange(U, device=dev), (rp[1:] - rp[:-1]).long())
    by_user = int((so[rows] < so[U + col.long()]).sum().item())
    emit(dict(base, entry="steps", t_best=t_best, n_best=n_best, density=round(f_best / (n_best * 2.0 ** 24), 6),
              block_users=int((so[:U] >= t_best).sum().item()), block_items=int((so[U:] >= t_best).sum().item()),
              user_steps_before_best=int((so[:U] < t_best).sum().item()), item_steps_before_best=int((so[U:] < t_best).sum().item()),
              edges_charged_from_user_steps=by_user, edges_charged_from_item_steps=nnz - by_user))
    dfd = model.from_config("defender", "FraudarSelectUsers", device=dev).I(dataset=(rp, col, val, I))
    dfd.defense_step()                                              # warm
    step_ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dfd.defense_step()
        torch.cuda.synchronize()
        step_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    emit(dict(base, entry="defense_step", ms=step_ms, n_flagged=int(dfd.predLabels.sum())))
    h_ptr, h_idx = rp.cpu().numpy().astype(np.int64), col.cpu().numpy().astype(np.int64)
    w = w_item.cpu().numpy().view(np.uint32)
    t0 = time.perf_counter()
    want = R.peel(U, I, h_ptr, h_idx, w)
    wall = time.perf_counter() - t0
    equal = bool(np.array_equal(want[0], first[0].cpu().numpy()) and np.array_equal(want[1], first[1].cpu().numpy())
                 and list(want[3]) == [t_best, f_best, n_best] and int(want[2][0]) == f_0)
    emit(dict(base, entry="python_heap_restatement", wall_s=round(wall, 3), device_words_equal=equal))
    if not equal:
        raise SystemExit("the restatement and the HIP path disagree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="tiny,ml1m,yelp")
    ap.add_argument("--timeout", type=float, default=500.0, help="seconds per shape")
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
