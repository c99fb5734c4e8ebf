"""AIA attacker timings (not the driver's bench line): for each synthetic shape (ml1m, yelp: recad_amd.synth interactions with
seeded 1..5 ratings, then partial_sample(user_ratio=0.2) as the reference's CLI does) and the reference's default
configuration, the wall time of one train_step split into the plain surrogate epochs, the unrolled epoch's forward, the
attack loss + reverse pass and the G step, plus us per WMF step.  It also times a dense PyTorch restatement of the same
train_step on the GPU (dense batches and P Q^T, autograd with create_graph through the unrolled epoch, no `higher`) as the
baseline: its plain epochs are timed over --dense-epochs and scaled to epoch_s.
Config 4 is skipped: ~12.5 K steps per epoch over ~700 K rows, 50 epochs per train_step.
Each shape runs in a child process of its own under its own time limit; one JSON line per shape.

    python scripts/bench_aia.py [--shapes ml1m,yelp] [--timeout 900] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _data(shape, dev):
    import numpy as np

    from recad_amd import dataset, synth

    d = synth.make_device(shape, dev)
    d = synth.with_ratings({k: (tuple(t.cpu().numpy() for t in v) if isinstance(v, tuple) else v) for k, v in d.items()})
    full = dataset.from_config("explicit", shape, train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], device=dev)
    np.random.seed(1)
    return full.partial_sample(user_ratio=0.2)


def dense_train_step_s(ds, att, dev, dense_epochs):
    """The reference's formulation (aia.py:88-114, 421-489) densely on the GPU: (plain epoch s, unrolled + loss + backward s)."""
    import numpy as np
    import torch

    U, I, A, R, d, B = att.n_users, att.n_items, att.attack_num, att.R, att.dim, att.batch
    ptr, idx, val = ds.rating_csr()
    X = torch.zeros(R, I, device=dev)
    X[torch.as_tensor(np.repeat(np.arange(U), np.diff(ptr))).to(dev), torch.as_tensor(idx.astype(np.int64)).to(dev)] = \
        torch.as_tensor(val).to(dev)
    fake = torch.zeros(A, I, device=dev)
    fake[torch.arange(A).repeat_interleave(att.filler_num).to(dev), torch.as_tensor(att.template_cols.reshape(-1)).to(dev)] = \
        torch.as_tensor(att.generator_values().reshape(-1)).to(dev)
    fake.requires_grad_(True)
    P = torch.zeros(R, d, device=dev).normal_(0, 0.1).requires_grad_(True)
    Q = torch.zeros(I, d, device=dev).normal_(0, 0.1).requires_grad_(True)
    opt = torch.optim.Adam([Q, P], lr=att.lr_s, weight_decay=att.wd_s)
    idx_list = np.arange(R)

    def plain_step(b):
        Xb = X[b]
        loss = ((Xb > 0).float() * (Xb - P[b] @ Q.t()) ** 2).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()

    warm = torch.as_tensor(idx_list[:B]).to(dev)
    for _ in range(3):               # untimed: the first hipBLAS GEMM, autograd backward and Adam step
        plain_step(warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(dense_epochs):
        np.random.shuffle(idx_list)
        for s in range(0, R, B):
            plain_step(torch.as_tensor(idx_list[s:s + B]).to(dev))
    torch.cuda.synchronize()
    plain = (time.perf_counter() - t0) / dense_epochs
    data = torch.cat([X[:U], fake], 0)
    Pf, Qf = P.detach().clone().requires_grad_(True), Q.detach().clone().requires_grad_(True)
    st = [opt.state[p] for p in (P, Q)]
    mP, vP, mQ, vQ = st[0]["exp_avg"].clone(), st[0]["exp_avg_sq"].clone(), st[1]["exp_avg"].clone(), st[1]["exp_avg_sq"].clone()
    t = int(st[0]["step"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    np.random.shuffle(idx_list)
    Pc, Qc = Pf, Qf
    for s in range(0, R, B):
        b = torch.as_tensor(idx_list[s:s + B]).to(dev)
        Xb = data[b]
        loss = ((Xb > 0).float() * (Xb - Pc[b] @ Qc.t()) ** 2).sum()
        gP, gQ = torch.autograd.grad(loss, (Pc, Qc), create_graph=True)
        t += 1
        bc1, bc2 = 1 - 0.9 ** t, 1 - 0.999 ** t
        gP, gQ = gP + att.wd_s * Pc, gQ + att.wd_s * Qc
        mP, mQ = 0.9 * mP + 0.1 * gP, 0.9 * mQ + 0.1 * gQ
        vP, vQ = 0.999 * vP + 0.001 * gP * gP, 0.999 * vQ + 0.001 * gQ * gQ
        Pc = Pc - att.lr_s / bc1 * mP / ((vP + 1e-30).sqrt() / bc2 ** 0.5 + 1e-8)
        Qc = Qc - att.lr_s / bc1 * mQ / ((vQ + 1e-30).sqrt() / bc2 ** 0.5 + 1e-8)
    sur = Pc @ Qc.t()
    tu = torch.as_tensor(np.where(X[:U, 0].cpu().numpy() == 0)[0]).to(dev)
    su = sur[tu]
    z = su * (su >= su[:, :1]).float()
    G = (-torch.log_softmax(z, -1)[:, 0] / 1.1).mean() / 10
    G.backward()
    torch.cuda.synchronize()
    return plain, time.perf_counter() - t0


def measure(shape, dense_epochs):
    import numpy as np
    import torch

    from recad_amd import model

    dev = torch.device("cuda:0")
    ds = _data(shape, dev)
    np.random.seed(3)
    torch.manual_seed(3)
    att = model.from_config("attacker", "aia", device=dev).I(dataset=ds)
    att.train_step(target_id_list=[0])              # warm-up (code objects, allocator)
    E, Ke, nb = att.epoch_s, att.unroll, att._nsteps()
    # the phases of one train_step, each closed by a synchronize
    att._project()
    theta0 = att.init_surrogate()
    perms, invs = att._perms(np.arange(att.R), E)
    dp, di = torch.as_tensor(perms).to(dev), torch.as_tensor(invs).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    state, t = att.run_plain(theta0, dp[: E - Ke], di[: E - Ke])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    K = Ke * nb
    hist = torch.empty(K + 1, state.numel(), device=dev)
    hist[0] = state
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for e, lo, hi, g in att._pieces(0, K):
        att._fwd(dp[E - Ke + e], di[E - Ke + e], lo, hi, t + g + 1, hist[g], True)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    del hist
    loss, xbar, _ = att.unrolled(state, t, dp[E - Ke:], di[E - Ke:], [0])
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    att.last_xbar = xbar
    att._g_t += 1
    from recad_amd import _lib
    _lib.check(_lib.lib().rk_aia_g_step(att.gen.numel(), _lib.ptr(att.gen), _lib.ptr(att.gen_m), _lib.ptr(att.gen_v), _lib.ptr(xbar),
                                        att._g_t, att.lr_g, 0.9, 0.999, 1e-8, att._s()), "rk_aia_g_step")
    att._project()
    torch.cuda.synchronize()
    t5 = time.perf_counter()
    reps = 3
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    for _ in range(reps):
        att.train_step(target_id_list=[0])
    torch.cuda.synchronize()
    whole = (time.perf_counter() - w0) / reps
    plain_steps = (E - Ke) * nb
    res = {"shape": shape, "n_rows": att.R, "n_items": att.n_items, "nnz": int(att._col.numel()), "steps_per_epoch": nb,
           "epoch_s": E, "unrolled_steps": K, "train_step_s": round(whole, 4),
           "plain_epochs_s": round(t1 - t0, 4), "unrolled_forward_s": round(t3 - t2, 4),
           "loss_and_reverse_s": round((t4 - t3) - (t3 - t2), 4), "g_step_s": round(t5 - t4, 5),
           "us_per_wmf_step": round((t1 - t0) / max(1, plain_steps) * 1e6, 2), "history_full": att.last_history["full"]}
    plain, unrolled = dense_train_step_s(ds, att, dev, dense_epochs)
    dense = plain * (E - Ke) + unrolled
    res.update({"dense_plain_epoch_s": round(plain, 4), "dense_unrolled_and_backward_s": round(unrolled, 4),
                "dense_train_step_s": round(dense, 3), "speedup_vs_dense": round(dense / whole, 1)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,yelp")
    ap.add_argument("--timeout", type=float, default=900.0, help="seconds per shape")
    ap.add_argument("--dense-epochs", type=int, default=2, help="plain epochs the dense baseline times (scaled to epoch_s)")
    ap.add_argument("--out", default=None, help="also write the results as one JSON list to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.child, a.dense_epochs)), flush=True)
        return 0
    results, rc = [], 0
    for shape in a.shapes.split(","):
        if shape == "config4":
            results.append({"shape": shape, "skipped": "about 12.5 K surrogate steps per epoch over ~700 K rows, 50 epochs per train_step"})
            print(json.dumps(results[-1]), flush=True)
            continue
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--dense-epochs", str(a.dense_epochs)],
                               capture_output=True, text=True, timeout=a.timeout, cwd=ROOT)
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
