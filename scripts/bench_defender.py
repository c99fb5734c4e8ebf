"""PCASelectUsers defender timings (not the driver's bench line): for each synthetic shape (ml1m, yelp, config4: the
train edges of recad_amd.synth.make_device, every value 1.0) the us per covariance application C.X (two narrow SpMMs,
block width 8), the subspace-iteration count, and the wall time of one whole defense_step (transpose, column scale,
solve, distances, selection).  Each shape runs in a child process of its own under its own time limit; one JSON line
per shape, and with --out all of them as one JSON file.

    python scripts/bench_defender.py [--shapes ml1m,yelp,config4] [--timeout 300] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(shape):
    sys.path.insert(0, ROOT)
    import torch

    from recad_amd import model, synth
    from recad_amd.defense.pca_select_users import CovarianceOperator

    dev = torch.device("cuda:0")
    d = synth.make_device(shape, dev)
    ptr, idx = d["train"]
    U, I = d["n_users"], d["n_items"]
    rp, val = ptr.to(torch.int32), torch.ones(idx.numel(), dtype=torch.float32, device=dev)
    out = {"shape": shape, "n_users": U, "n_items": I, "nnz": int(idx.numel())}
    op = CovarianceOperator(U, I, rp, idx, val)
    for b in (8, 16):
        X = torch.randn(I, b, device=dev)
        Y = torch.empty_like(X)
        for _ in range(3):
            op.apply(X, Y)
        reps = 20
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            op.apply(X, Y)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        # bytes of one application: two passes over (col int32 + val fp32) + the gathered rows (4 b bytes per nonzero) +
        # the output rows
        nnz = idx.numel()
        byt = 2 * nnz * (8 + 4 * b) + (U + I) * 4 * b
        out[f"us_per_CX_b{b}"] = round(us, 1)
        out[f"gather_GBs_b{b}"] = round(byt / us / 1e3, 1)
    del op
    dfd = model.from_config("defender", "PCASelectUsers", attack_num=50, device=dev).I(dataset=(rp, idx, val, I))
    dfd.defense_step()                                                # warm (allocator, code objects)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    spam = dfd.defense_step()
    torch.cuda.synchronize()
    out["defense_step_s"] = round(time.perf_counter() - t0, 3)
    out["iterations"] = dfd.iterations
    out["eigenvalues"] = [round(float(v), 3) for v in dfd.eigenvalues]
    out["n_flagged"] = len(spam)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,yelp,config4")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per shape")
    ap.add_argument("--out", default=None, help="also write the results as one JSON list to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.child)), flush=True)
        return 0
    results, rc = [], 0
    for shape in a.shapes.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape], capture_output=True, text=True,
                               timeout=a.timeout, cwd=ROOT)
        except subprocess.TimeoutExpired:
            results.append({"shape": shape, "error": f"time limit {a.timeout:.0f} s"})
            print(json.dumps(results[-1]), flush=True)
            rc = 1
            break
        if p.returncode != 0:
            results.append({"shape": shape, "error": f"exit {p.returncode}", "stderr": p.stderr[-2000:]})
            print(json.dumps(results[-1]), flush=True)
            rc = 1
            break                   # a failed GPU child ends the run: nothing more is started on the card
        line = p.stdout.strip().splitlines()[-1]
        results.append(json.loads(line))
        print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
