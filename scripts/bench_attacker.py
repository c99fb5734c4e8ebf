"""AUSH attacker timings (not the driver's bench line): for each synthetic shape (ml1m, yelp, config4: recad_amd.synth
interactions with seeded 1..5 ratings, then partial_sample(user_ratio=0.2) as the reference's CLI does) the wall time of
one train_step epoch and per batch, of one generate_fake, and the bytes one discriminator Adam step moves.  At ml1m and
yelp it also times a dense PyTorch restatement of the same epoch on the GPU (dense B x I batches, nn.Linear layers,
autograd, torch.optim.Adam: the reference's formulation, aush.py:79-175) as the "reference on this GPU" baseline.
Each shape runs in a child process of its own under its own time limit; one JSON line per shape.

With --kernel-stats FILE --results FILE --shape S (the kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of
`bench_attacker.py --child S`, and the JSON list of an earlier --out run), the average duration of the Adam kernel is
read from it and its bytes over time are reported as a share of the 8 TB/s HBM peak (an upper bound: see below).

    python scripts/bench_attacker.py [--shapes ml1m,yelp,config4] [--timeout 600] [--out FILE]
    python scripts/bench_attacker.py --kernel-stats FILE --results FILE --shape yelp
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12


def _data(shape, dev):
    import numpy as np

    from recad_amd import dataset, synth

    d = synth.make_device(shape, dev)
    d = synth.with_ratings({k: (tuple(t.cpu().numpy() for t in v) if isinstance(v, tuple) else v) for k, v in d.items()})
    full = dataset.from_config("explicit", shape, train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], device=dev)
    np.random.seed(1)
    return full.partial_sample(user_ratio=0.2)


def dense_epoch_s(ds, dev, att, n_batches):
    """The reference's train_step formulation, dense, on the GPU, for n_batches batches of the same size."""
    import numpy as np
    import torch
    from torch import nn

    I, B, F = ds.n_items, att.batch_size, att.filler_num
    S = att._sel_host.tolist()
    ptr, idx, val = ds.rating_csr()
    rows = torch.as_tensor(np.repeat(np.arange(ds.n_users), np.diff(ptr))).to(dev)
    cols, vals = torch.as_tensor(idx.astype(np.int64)).to(dev), torch.as_tensor(val).to(dev)
    netG = nn.Sequential(nn.Linear(I, 128), nn.Sigmoid(), nn.Linear(128, I), nn.Sigmoid()).to(dev)
    netD = nn.Sequential(nn.Linear(I, 150), nn.Sigmoid(), nn.Linear(150, 150), nn.Sigmoid(), nn.Linear(150, 150), nn.Sigmoid(),
                         nn.Linear(150, 1), nn.Sigmoid()).to(dev)
    optD = torch.optim.Adam(netD.parameters(), lr=1e-3)
    bce, mse = nn.BCELoss(), nn.MSELoss()
    el = torch.as_tensor(att.eligible_users([0]).astype(np.int64)).to(dev)
    sel = torch.zeros(B, I, device=dev)
    sel[:, S] = 1.0

    def one():
        users = el[torch.randint(0, el.numel(), (B,), device=dev)]
        real = torch.zeros(B, I, device=dev)
        pos = torch.searchsorted(users.sort().values, rows)     # dense rows of the batch (train_mat[users])
        m = torch.isin(rows, users)
        real[pos[m], cols[m]] = vals[m]
        fill = (torch.rand(B, I, device=dev) < F / 200.0).float() * (real > 0).float() * (1 - sel)
        zr = (real == 0).float() * sel
        tmpl = real * fill
        gen = netG(tmpl).detach() * 5
        fake = tmpl + gen * sel + 5 * sel
        optD.zero_grad()
        mask = fill + sel
        d_loss = 0.5 * (bce(netD(real * mask), torch.ones(B, 1, device=dev)) + bce(netD(fake * mask), torch.zeros(B, 1, device=dev)))
        d_loss.backward()
        optD.step()
        g = bce(netD(fake * mask), torch.ones(B, 1, device=dev)) + mse(fake * sel, sel * 5) + mse(fake * sel * zr, sel * tmpl * zr)
        return d_loss.item(), g.item()

    one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_batches):
        one()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def measure(shape):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from recad_amd import model

    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    ds = _data(shape, dev)
    out = {"shape": shape, "n_users": ds.n_users, "n_items": ds.n_items, "nnz": int(ds.rating_csr()[0][-1]),
           "data_s": round(time.perf_counter() - t0, 1)}
    torch.manual_seed(0)
    t0 = time.perf_counter()
    att = model.from_config("attacker", "aush", device=dev, seed=1).I(dataset=ds)
    torch.cuda.synchronize()
    out["init_s"] = round(time.perf_counter() - t0, 2)
    att.train_step(target_id_list=[0])                     # warm: pool, buffers, code objects
    torch.cuda.synchronize()
    reps = 3
    t0 = time.perf_counter()
    for _ in range(reps):
        att.train_step(target_id_list=[0])
    torch.cuda.synchronize()
    ep = (time.perf_counter() - t0) / reps
    nb = att.last_batch_losses.shape[0]
    out.update(eligible=int(att._pools[(0,)]["n"]), batches=nb, epoch_ms=round(ep * 1e3, 2), batch_us=round(ep / nb * 1e6, 1))
    att.generate_fake(target_id_list=[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fake = att.generate_fake(target_id_list=[0])
    out["generate_fake_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    out["fake_shape"] = list(fake.shape)
    touched = int(att._n_touched.item())
    tail = 150 + 150 * 150 + 150 + 150 * 150 + 150 + 150 + 1
    # per Adam element: read p, m, v, g; write p, m, v (the first-layer gradient is read through its slot)
    out["adam_rows_touched"] = touched
    out["adam_bytes_per_step"] = (touched * 150 + tail) * 4 * 7
    out["adam_dense_bytes_per_step"] = (ds.n_items * 150 + tail) * 4 * 7
    if shape in ("ml1m", "yelp"):
        dense = dense_epoch_s(ds, dev, att, nb)
        out["dense_torch_epoch_ms"] = round(dense * 1e3, 2)
        out["speedup_vs_dense_torch"] = round(dense / ep, 2)
    out["losses_finite"] = bool(np.isfinite(att.last_batch_losses).all())
    return out


def adam_kernel_us(path):
    with open(path) as f:
        for row in csv.DictReader(f):
            if "d_adam_kernel" in row.get("Name", ""):
                return float(row["AverageNs"]) / 1e3
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,yelp,config4")
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds per shape")
    ap.add_argument("--out", default=None, help="also write the results as one JSON list to this file")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this script (one shape)")
    ap.add_argument("--results", default=None, help="with --kernel-stats: the JSON list an earlier run wrote with --out")
    ap.add_argument("--shape", default="yelp", help="with --kernel-stats: the shape the profiled run measured")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.child)), flush=True)
        return 0
    if a.kernel_stats:
        us = adam_kernel_us(a.kernel_stats)
        res = json.load(open(a.results)) if a.results else []
        for r in res:
            if us and r.get("shape") == a.shape and "adam_bytes_per_step" in r:
                # adam_bytes_per_step counts the rows touched at the END of the run, the kernel average spans every step
                # (early steps touch fewer rows): the share is an upper bound
                print(json.dumps({"shape": r["shape"], "adam_kernel_us_avg": round(us, 2),
                                  "adam_GBs_upper": round(r["adam_bytes_per_step"] / us / 1e3, 1),
                                  "adam_share_of_hbm_peak_upper": round(r["adam_bytes_per_step"] / (us * 1e-6) / HBM_PEAK, 3)}))
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
