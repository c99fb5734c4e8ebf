"""APR victim timings (not the driver's bench line): rk_apr_train_epoch at the ml1m shape (5 950 x 3 702, d = 64, B = 1024) and the
yelp shape (54 632 x 34 474, d = 128, B = 1024), for adv_reg = 0 (plain BPR-MF: three launches per step) and adv_reg = 1 (five).
Triplets: `--steps` * B train edges of recad_amd.synth.make_device(shape) drawn at random, the negative a uniform item (it is not
checked against the user's row: this is a timing shape, and the run lengths of the plan come from the real degrees).

What is timed.  Whole calls by device events after two warm calls, `--reps` of them, reported as median / min / max: a call is the
id check with its one read-back, the plan (keys, one radix sort, the run table) and the steps, so us_per_step is the call over
the steps and includes them.  The comparator is timed the same way over max(3, reps // 2) calls after ONE warm call.  The split per kernel and the plan's share come from a separate run under
`rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/bench_apr.py --reps 3 --no-comparator`, with nothing else
traced in it: the library call has no seam to put an event into.

The comparator runs in the same process on the same card: the same step composed from what the library had before
(rk_bpr_rows_ordered with n_layers = 0 twice, torch ops for the row gathers, the row norms and the moved table,
rk_adam_coef_advance and rk_adam_step_dev), with the epoch's keys sorted beforehand OUTSIDE the timed window.  It computes the same
step up to rounding (its Delta and Adam are dense, its sums in another order); the script prints how far the two tables end apart.

Counted bytes per step, so a reader can see how far a step is from a streaming bound: the dense Adam pass reads and writes p, m and v and reads
and clears g, 8 words an element, 32 N d bytes, of which p, m and v are 24 N d (both are reported); the row gathers move 4 d B words times 3
(coefficients) + 4 (Gamma: two partner rows for the user, one per item) + 6 (moved rows and their Deltas) + 11 (gradient: partners,
their Deltas, the row itself) = 96 d B bytes with adv_reg != 0, 4 d B * (3 + 7) = 40 d B without.

    python scripts/bench_apr.py [--shape ml1m|yelp] [--steps 200] [--reps 7] [--no-comparator] [--out profiles/bench_apr_mi355x.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = {"ml1m": 64, "yelp": 128}
LAM, EPS, LR, B1, B2, ADAM_EPS = 1e-4, 0.5, 1e-3, 0.9, 0.999, 1e-8


def _timed(fn, reps, warm=2):
    import torch

    times = []
    for r in range(reps + warm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= warm:
            times.append(e0.elapsed_time(e1))
    return {"median": statistics.median(times), "min": min(times), "max": max(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml1m", choices=sorted(DIMS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-comparator", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_apr_mi355x.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    from recad_amd import _lib, synth

    _lib.require_gpu()
    dev = torch.device("cuda:0")
    data = synth.make_device(args.shape, dev)
    U, I, d, B, S = data["n_users"], data["n_items"], DIMS[args.shape], args.batch, args.steps
    N, n = U + I, args.steps * args.batch
    ptr, idx = data["train"]
    gen = torch.Generator(device=dev).manual_seed(1)
    edge = torch.randint(0, idx.numel(), (n,), device=dev, generator=gen)
    users = (torch.searchsorted(ptr.long(), edge, right=True) - 1).contiguous()
    pos = idx.long()[edge].contiguous()
    neg = torch.randint(0, I, (n,), device=dev, generator=gen)
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    tab0 = torch.randn(N, d, device=dev, generator=gen) * 0.1

    lay = _lib.AprLayout()
    _lib.check(L.rk_apr_workspace(U, I, d, n, B, C.byref(lay)), "rk_apr_workspace")
    ws = torch.empty(lay.bytes, dtype=torch.uint8, device=dev)
    losses = torch.empty(3 * S, dtype=torch.float64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    state = {}

    def fresh():
        state["tab"], state["m"], state["v"] = tab0.clone(), torch.zeros_like(tab0), torch.zeros_like(tab0)

    def epoch(adv_reg):
        desc = _lib.AprDesc(n_users=U, n_items=I, dim=d, table=state["tab"].data_ptr(), m=state["m"].data_ptr(), v=state["v"].data_ptr(), grad=None,
                            lam=LAM, eps=EPS, adv_reg=adv_reg, lr=LR, beta1=B1, beta2=B2, adam_eps=ADAM_EPS, workspace=ws.data_ptr(),
                            workspace_bytes=ws.numel())
        _lib.check(L.rk_apr_train_epoch(C.byref(desc), P(users), P(pos), P(neg), n, B, 0, 1, P(losses), P(status), s), "rk_apr_train_epoch")

    out = {"shape": args.shape, "n_users": U, "n_items": I, "dim": d, "batch": B, "steps": S, "reps": args.reps,
           "workspace_bytes": int(lay.bytes), "adam_bytes_per_step": 32 * N * d, "adam_bytes_per_step_p_m_v": 24 * N * d, "gather_bytes_per_step_adv": 96 * d * B,
           "gather_bytes_per_step_bpr": 40 * d * B}
    for name, adv in (("bpr", 0.0), ("apr", 1.0)):
        fresh()
        t = _timed(lambda: epoch(adv), args.reps)
        out[f"{name}_us_per_step"] = {k: round(v * 1e3 / S, 2) for k, v in t.items()}
        out[f"{name}_losses_last_step"] = [round(float(x), 6) for x in losses[-3:].cpu()]
    # one epoch from tab0 for the comparison below
    fresh()
    epoch(1.0)
    torch.cuda.synchronize()
    lib_tab = state["tab"].clone()

    if not args.no_comparator:
        rows_u, rows_p, rows_n = users, pos + U, neg + U
        inc = (3 * torch.arange(B, device=dev)[:, None] + torch.arange(3, device=dev)[None, :]).reshape(1, -1)
        rows3 = torch.stack([rows_u, rows_p, rows_n], dim=1).reshape(S, 3 * B)
        keys = torch.sort((rows3 << 20) | inc, dim=1).values.contiguous()                 # outside the timed window
        flat = torch.cat([rows_u.view(S, B), rows_p.view(S, B), rows_n.view(S, B)], dim=1).contiguous()      # [S, 3 B]: users, positives, negatives
        gprop1, gego1, gprop2, gego2 = (torch.zeros(N, d, device=dev) for _ in range(4))
        lp = torch.empty(_lib.RK_LOSS_PARTIALS, device=dev)
        coef, counter = torch.zeros(2, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

        def bpr(lam, light, gp, ge, st):
            sl = slice(st * B, (st + 1) * B)
            _lib.check(L.rk_bpr_rows_ordered(d, 0, lam, P(light), P(state["tab"]), P(gp), P(ge), P(rows_u[sl]), P(rows_p[sl]), P(rows_n[sl]), B,
                                             P(keys[st]), P(lp), s), "rk_bpr_rows_ordered")

        def composed():
            counter.zero_()
            tab, m, v = state["tab"], state["m"], state["v"]
            for st in range(S):
                bpr(LAM, tab.index_select(0, flat[st]), gprop1, gego1, st)
                norms = gprop1.norm(dim=1, keepdim=True).clamp_min_(1e-12)
                moved = torch.addcdiv(tab, gprop1, norms, value=EPS)
                bpr(0.0, moved.index_select(0, flat[st]), gprop2, gego2, st)
                gego1.add_(gprop2)
                _lib.check(L.rk_adam_coef_advance(P(coef), P(counter), LR, B1, B2, s), "rk_adam_coef_advance")
                _lib.check(L.rk_adam_step_dev(N * d, P(tab), P(gego1), P(m), P(v), P(coef), B1, B2, ADAM_EPS, s), "rk_adam_step_dev")
                gprop1.zero_(); gego1.zero_(); gprop2.zero_(); gego2.zero_()

        fresh()
        t = _timed(composed, max(3, args.reps // 2), warm=1)
        out["composed_reps"] = max(3, args.reps // 2)
        out["composed_us_per_step"] = {k: round(v * 1e3 / S, 2) for k, v in t.items()}
        out["composed_over_apr"] = round(t["median"] * 1e3 / S / out["apr_us_per_step"]["median"], 3)
        fresh()
        composed()
        torch.cuda.synchronize()
        out["max_abs_table_difference_after_one_epoch"] = float((state["tab"] - lib_tab).abs().max())
        out["max_abs_table_move_after_one_epoch"] = float((lib_tab - tab0).abs().max())
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
