"""KnnSelectUsers defender timings (not the driver's bench line): for each synthetic shape (ml1m, yelp: the train edges of
recad_amd.synth.make_device), with every value 1.0 ("implicit") and with seeded 1..5 ratings ("ratings"), the wall time of
one whole defense_step (norms, transpose, work order, DegSim, selection; a host clock around work that ends in a device
synchronise) and the device-event time of rk_knn_degsim alone, for schedule work / natural and band automatic / 4096.

Counted work: adds = sum_i deg(i)^2 integer LDS atomic adds per call (every pair of users that share item i, both ways,
the self pair included; it does not depend on the band), lds_GBs = 4 bytes per add over the kernel time.  Neither is a
share of peak: no LDS-atomic rate is documented for this part.

The comparator is the dense formulation in PyTorch on the same card in the same run: the row-normalised dense A, A @ A.T,
torch.topk k + 1 wide with the self column dropped, mean.  It needs 4 U^2 + 4 U I bytes and is not bit-exact.

Each shape runs in a child process of its own under its own time limit; one JSON line per measurement, appended to --out.

    python scripts/bench_knn_defender.py [--shapes ml1m,yelp] [--timeout 400] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 25


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


def measure(shape, emit):
    sys.path.insert(0, ROOT)
    import torch

    from recad_amd import _lib, model, synth
    from recad_amd.defense.knn_select_users import work_order

    dev = torch.device("cuda:0")
    d = synth.make_device(shape, dev)
    ptr, idx = d["train"]
    U, I = d["n_users"], d["n_items"]
    rp, idx = ptr.to(torch.int32).contiguous(), idx.to(torch.int32).contiguous()
    nnz = int(idx.numel())
    deg = torch.bincount(idx.long(), minlength=I).double()
    adds = float((deg * deg).sum().item())
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    ratings = torch.clamp(torch.round(3.6 + 1.1 * torch.randn(nnz, device=dev, generator=g)), 1, 5).float()
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    base = {"shape": shape, "n_users": U, "n_items": I, "nnz": nnz, "k": K, "lds_adds": adds}
    for values, val in (("implicit", torch.ones(nnz, dtype=torch.float32, device=dev)), ("ratings", ratings)):
        rnorm = torch.empty(U, dtype=torch.float32, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        _lib.check(L.rk_knn_norms(U, I, P(rp), P(idx), P(val), P(rnorm), P(status), s), "rk_knn_norms")
        colptr = torch.empty(I + 1, dtype=torch.int32, device=dev)
        crow, cval = torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.float32, device=dev)
        _lib.check(L.rk_pca_transpose(U, I, P(rp), P(idx), P(val), P(colptr), P(crow), P(cval), s), "rk_pca_transpose")
        order = work_order(rp, idx, colptr)
        topw = torch.empty(U, K, dtype=torch.float32, device=dev)
        degsim = torch.empty(U, dtype=torch.float32, device=dev)
        first = None
        for schedule in ("work", "natural"):
            for band in (0, 4096):
                def call():
                    _lib.check(L.rk_knn_degsim(U, I, P(rp), P(idx), P(val), P(colptr), P(crow), P(cval), P(rnorm), K, band,
                                               P(order) if schedule == "work" else None, P(topw), P(degsim), s), "rk_knn_degsim")
                call()                                                    # warm
                torch.cuda.synchronize()
                if first is None:
                    first = (topw.clone(), degsim.clone())
                same = bool(torch.equal(first[0], topw) and torch.equal(first[1], degsim))
                ms = _events(call)
                dfd = model.from_config("defender", "KnnSelectUsers", k=K, attack_num=50, schedule=schedule, band=band or None,
                                        device=dev).I(dataset=(rp, idx, val, I))
                dfd.defense_step()                                        # warm
                torch.cuda.synchronize()
                n_steps = 50 if shape == "ml1m" else 10
                t0 = time.perf_counter()
                for _ in range(n_steps):
                    dfd.defense_step()
                torch.cuda.synchronize()
                step_ms = (time.perf_counter() - t0) / n_steps * 1e3
                emit(dict(base, values=values, path="hip", schedule=schedule, band=band or "auto", degsim_kernel_ms=round(ms, 3),
                          defense_step_ms=round(step_ms, 3), lds_adds_per_s=round(adds / (ms * 1e-3), 0),
                          lds_GBs=round(4 * adds / (ms * 1e-3) / 1e9, 1), same_bits_as_first=same))
        # the dense formulation in torch on the same card
        def dense():
            A = torch.zeros(U, I, dtype=torch.float32, device=dev)
            rows = torch.repeat_interleave(torch.arange(U, device=dev), (rp[1:] - rp[:-1]).long())
            A[rows, idx.long()] = val
            A = A / A.norm(dim=1, keepdim=True).clamp_min(1e-30)
            S = A @ A.T
            S.fill_diagonal_(float("-inf"))
            top = torch.topk(S, K + 1, dim=1).values[:, :K]               # k + 1 wide; the self column sorts last and is dropped
            return top.clamp_min(0).mean(dim=1)
        try:
            ref = dense()                                                 # warm
            torch.cuda.synchronize()
            ms = _events(dense, 1.0)
            err = float((ref - first[1]).abs().max().item())
            emit(dict(base, values=values, path="torch-dense", dense_ms=round(ms, 3), max_abs_diff_to_hip=err,
                      dense_bytes=4 * U * U + 4 * U * I))
            del ref
        except torch.OutOfMemoryError as e:
            emit(dict(base, values=values, path="torch-dense", error=f"out of memory: {str(e)[:120]}"))
        torch.cuda.empty_cache()


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
