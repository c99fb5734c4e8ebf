"""Heuristic attacker kernel timings (not the driver's bench line): rk_heur_item_stats and rk_heur_generate on the train
ratings of the synthetic ml1m and yelp shapes (recad_amd.synth interactions with seeded 1..5 ratings), device events around
each call, the median of --reps calls after --warmup, and the share of the 8 TB/s HBM peak the call's minimum bytes make:

    item_stats  nnz * (4 + 4) for the first pass (item id, rating), nnz * 4 for the second (rating), n_items * (4 + 8) * 2
                for zeroing and finishing the per-item arrays; the float64 / int32 atomics' own traffic is not counted
    generate    attack_num * n_items * 4 written (the few nonzeros rewrite lines already counted)

A call is several launches (item_stats: three zero fills, two passes, two one-block reductions, one finish), so at these
sizes the time holds launch gaps as well as kernel time: it is the call's time, not a kernel's.  One JSON line per shape.

    python scripts/bench_heuristic.py [--shapes ml1m,yelp] [--attack-num 50] [--filler-num 36] [--reps 50] [--warmup 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12


def _median_ms(fn, reps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def measure(shape, attack_num, filler_num, reps, warmup):
    import torch

    from recad_amd import _lib, synth

    dev = torch.device("cuda:0")
    d = synth.make_device(shape, dev)
    ptr, idx = d["train"]
    I, nnz = int(d["n_items"]), int(idx.numel())
    col = idx.to(torch.int32).contiguous()
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    val = torch.clamp(torch.round(3.6 + 1.1 * torch.randn(nnz, device=dev, generator=g)), 1, 5).to(torch.float32)
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    cnt = torch.empty(I, dtype=torch.int32, device=dev)
    mean = torch.empty(I, dtype=torch.float64, device=dev)
    glob = torch.empty(2, dtype=torch.float64, device=dev)
    nr = torch.empty(1, dtype=torch.int32, device=dev)
    out = torch.empty(attack_num, I, dtype=torch.float32, device=dev)
    tg = (C.c_int32 * 1)(0)

    def stats():
        _lib.check(L.rk_heur_item_stats(I, nnz, P(col), P(val), P(cnt), P(mean), P(glob), P(nr), S), "rk_heur_item_stats")

    stats()
    gm, gs = (float(x) for x in glob.cpu().numpy())
    assert int(cnt.sum().item()) == nnz and abs(gm - float(val.double().mean().item())) < 1e-9

    def generate():
        _lib.check(L.rk_heur_generate(attack_num, I, filler_num, tg, 1, None, 0, _lib.RK_HEUR_ITEM, gm, gs, P(mean), P(cnt), None, None,
                                      1, 1 << 62, P(out), S), "rk_heur_generate")

    res = {"shape": shape, "n_users": int(d["n_users"]), "n_items": I, "nnz": nnz, "attack_num": attack_num, "filler_num": filler_num,
           "reps": reps, "warmup": warmup}
    for name, fn, nbytes in (("item_stats", stats, nnz * 12 + I * 24), ("generate", generate, attack_num * I * 4)):
        med, lo, hi = _median_ms(fn, reps, warmup)
        res[name] = {"median_us": round(med * 1e3, 1), "min_us": round(lo * 1e3, 1), "max_us": round(hi * 1e3, 1), "min_bytes": nbytes,
                     "GBs": round(nbytes / (med * 1e-3) / 1e9, 1), "share_of_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}
    assert int((out != 0).sum().item()) == attack_num * (filler_num + 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,yelp")
    ap.add_argument("--attack-num", type=int, default=50)
    ap.add_argument("--filler-num", type=int, default=36)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the results as one JSON list to this file")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    results = []
    for shape in a.shapes.split(","):
        results.append(measure(shape, a.attack_num, a.filler_num, a.reps, a.warmup))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
