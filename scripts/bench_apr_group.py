"""Grouped APR epoch against the single entry (not the driver's bench line): rk_apr_train_epoch_group over R models against R calls
of rk_apr_train_epoch, in the same process on the same card, at the ml1m shape (5 950 x 3 702, d = 64, B = 1024), for
R in {1, 2, 4, 8, 16}, as BPR (adv_reg = 0: three launches per step) and with the adversarial term (adv_reg = 1: five).

Members.  Member r is the clean set plus 50 r injected users (ids U .. U + 50 r - 1) of 37 items each, as a poisoning study
retrains them: its table has 50 r more rows and its epoch 1 850 r more triplets, so the members' step counts differ (`--steps` * B
triplets for member 0) and the group's last launches carry fewer members.  Triplets as in scripts/bench_apr.py: train edges of
recad_amd.synth.make_device("ml1m") drawn at random, the injected users' items and every negative uniform.

Before anything is timed, both paths run one epoch from the same tables and every member's table, m and v must be equal bit for
bit; a difference ends the run with exit status 1.

What is timed.  Device events around a window of `--reps` whole calls (the id check with its read-back, the plans, the steps)
after one warm call; the window is taken three times per (mode, R, path), grouped and single in turn.  us_per_member_step is the
window over reps * (the sum of the members' step counts): what one model's step costs.  `spread` is (max - min) / median of the
three windows.  Each mode runs in a child process of its own under its own time limit, and a failed child ends the run: nothing
more is started on the card.

    python scripts/bench_apr_group.py [--steps 200] [--reps 5] [--sizes 1,2,4,8,16] [--timeout 300] [--out profiles/bench_apr_group_mi355x.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, LAM, EPS, LR, B1, B2, ADAM_EPS = 64, 1e-4, 0.5, 1e-3, 0.9, 0.999, 1e-8
FAKE_PER_MEMBER, FAKE_ITEMS = 50, 37


def _window(fn, reps):
    import torch

    fn()                                            # the warm call
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps               # ms per call


def measure(mode, sizes, steps, batch, reps, emit):
    sys.path.insert(0, ROOT)
    import torch

    from recad_amd import _lib, synth

    _lib.require_gpu()
    dev = torch.device("cuda:0")
    data = synth.make_device("ml1m", dev)
    U, I, B = data["n_users"], data["n_items"], batch
    ptr, idx = data["train"]
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    adv_reg = 0.0 if mode == "bpr" else 1.0
    gen = torch.Generator(device=dev).manual_seed(1)

    def member(r):
        """the inputs of member r: sizes, triplets, the initial table"""
        n_clean, n_fake = steps * B, FAKE_PER_MEMBER * FAKE_ITEMS * r
        edge = torch.randint(0, idx.numel(), (n_clean,), device=dev, generator=gen)
        users = torch.searchsorted(ptr.long(), edge, right=True) - 1
        pos = idx.long()[edge]
        if n_fake:
            users = torch.cat([users, U + torch.arange(FAKE_PER_MEMBER * r, device=dev).repeat_interleave(FAKE_ITEMS)])
            pos = torch.cat([pos, torch.randint(0, I, (n_fake,), device=dev, generator=gen)])
        n = n_clean + n_fake
        perm = torch.randperm(n, device=dev, generator=gen)
        Ur = U + FAKE_PER_MEMBER * r
        return {"U": Ur, "n": n, "users": users[perm].contiguous(), "pos": pos[perm].contiguous(),
                "neg": torch.randint(0, I, (n,), device=dev, generator=gen), "tab0": torch.randn(Ur + I, D, device=dev, generator=gen) * 0.1,
                "n_steps": (n + B - 1) // B}

    def buffers(mb):
        """tables, moments, workspace, losses of one member for one path"""
        lay = _lib.AprLayout()
        _lib.check(L.rk_apr_workspace(mb["U"], I, D, mb["n"], B, C.byref(lay)), "rk_apr_workspace")
        b = {"tab": mb["tab0"].clone(), "m": torch.zeros_like(mb["tab0"]), "v": torch.zeros_like(mb["tab0"]),
             "ws": torch.empty(lay.bytes, dtype=torch.uint8, device=dev), "losses": torch.empty(3 * mb["n_steps"], dtype=torch.float64, device=dev)}
        b["desc"] = _lib.AprDesc(n_users=mb["U"], n_items=I, dim=D, table=b["tab"].data_ptr(), m=b["m"].data_ptr(), v=b["v"].data_ptr(), grad=None,
                                 lam=LAM, eps=EPS, adv_reg=adv_reg, lr=LR, beta1=B1, beta2=B2, adam_eps=ADAM_EPS, workspace=b["ws"].data_ptr(),
                                 workspace_bytes=b["ws"].numel())
        return b

    members = [member(r) for r in range(max(sizes))]
    for R in sizes:
        mbs = members[:R]
        one, grp = [buffers(mb) for mb in mbs], [buffers(mb) for mb in mbs]
        status1, statusR = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2 * R, dtype=torch.int32, device=dev)
        descs = (_lib.AprDesc * R)(*[b["desc"] for b in grp])
        arr = lambda ts: (C.c_void_p * R)(*[t.data_ptr() for t in ts])
        ga = (arr([mb["users"] for mb in mbs]), arr([mb["pos"] for mb in mbs]), arr([mb["neg"] for mb in mbs]), (C.c_int64 * R)(*[mb["n"] for mb in mbs]),
              (C.c_int32 * R)(*([0] * R)), arr([b["losses"] for b in grp]))

        def singles():
            for mb, b in zip(mbs, one):
                _lib.check(L.rk_apr_train_epoch(C.byref(b["desc"]), P(mb["users"]), P(mb["pos"]), P(mb["neg"]), mb["n"], B, 0, 1, P(b["losses"]),
                                                P(status1), s), "rk_apr_train_epoch")

        def grouped():
            _lib.check(L.rk_apr_train_epoch_group(R, descs, ga[0], ga[1], ga[2], ga[3], B, ga[4], 1, ga[5], P(statusR), s), "rk_apr_train_epoch_group")

        singles()
        grouped()
        torch.cuda.synchronize()
        for r, (a, b) in enumerate(zip(one, grp)):
            if not all(torch.equal(a[k], b[k]) for k in ("tab", "m", "v", "losses")):
                raise SystemExit(f"{mode} R = {R}: member {r} of the grouped epoch differs from the single entry's")
        wins = {"single": [], "group": []}
        for _ in range(3):
            wins["group"].append(_window(grouped, reps))
            wins["single"].append(_window(singles, reps))
        total_steps = sum(mb["n_steps"] for mb in mbs)
        rec = {"mode": mode, "R": R, "dim": D, "batch": B, "n_users": U, "n_items": I, "reps": reps, "member_steps": [mb["n_steps"] for mb in mbs],
               "tables_equal_bit_for_bit": True}
        for k, w in wins.items():
            med = statistics.median(w)
            rec[f"{k}_ms_per_epoch_windows"] = [round(x, 3) for x in w]
            rec[f"{k}_us_per_member_step"] = round(med * 1e3 / total_steps, 2)
            rec[f"{k}_spread"] = round((max(w) - min(w)) / med, 4)
        rec["single_over_group"] = round(statistics.median(wins["single"]) / statistics.median(wins["group"]), 3)
        emit(rec)
        del one, grp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,2,4,8,16")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per mode")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_apr_group_mi355x.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    if a.child:
        measure(a.child, sizes, a.steps, a.batch, a.reps, lambda rec: print(json.dumps(rec), flush=True))
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for mode in ("bpr", "apr"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--steps", str(a.steps), "--batch", str(a.batch), "--reps", str(a.reps),
                   "--sizes", a.sizes]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, cwd=ROOT)
                lines, err = p.stdout, (None if p.returncode == 0 else f"exit {p.returncode}: {p.stderr[-1500:]}")
            except subprocess.TimeoutExpired as e:
                lines, err = (e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")), f"time limit {a.timeout:.0f} s"
            for line in lines.strip().splitlines():
                if line.startswith("{"):
                    print(line, flush=True)
                    out.write(line + "\n")
                    out.flush()
            if err:
                print(json.dumps({"mode": mode, "error": err}), flush=True)
                return 1                # a failed GPU child ends the run: nothing more is started on the card
    return 0


if __name__ == "__main__":
    sys.exit(main())
