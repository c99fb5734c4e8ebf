"""AushPlus attacker timings (not the driver's bench line): for each synthetic shape (ml1m, yelp: recad_amd.synth interactions
with seeded 1..5 ratings, then partial_sample(user_ratio=0.2) as the reference's CLI does) and the reference's default
configuration, the wall time of one train_step split by phase: pretrain (pretrain_G + its train_D epochs, first step only),
the GAN's D epochs, the adversarial G epoch and the surrogate phase (epoch_surrogate fits, timed over --fits of them and scaled).
It also times a dense PyTorch restatement of phases 1-3 on the same GPU (dense batch x I rows through nn.Linear layers, the
projection over all I columns, autograd), warmed up first; the dense surrogate fit is scripts/bench_aia.py's baseline.
Each shape runs in a child process of its own under its own time limit; one JSON line per shape.

    python scripts/bench_aushplus.py [--shapes ml1m,yelp] [--fits 3] [--timeout 600] [--out FILE]
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

    r = synth.with_ratings(synth.make(shape))
    full = dataset.from_config("explicit", shape, train_csr=r["train"], valid_csr=r["valid"], test_csr=r["test"], device=dev)
    np.random.seed(1)
    return full.partial_sample(user_ratio=0.2)


def dense_phases_s(att, dev):
    """Phases 1-3 as the reference runs them, densely on the GPU: (pretrain_G epoch, train_D epoch, train_G adv) seconds."""
    import numpy as np
    import torch
    from torch import nn

    U, I, A, bs = att.n_users, att.n_items, att.attack_num, att.batch_size
    ptr, idx, val = att._host_csr
    X = torch.zeros(U, I, device=dev)
    X[torch.as_tensor(np.repeat(np.arange(U), np.diff(ptr))).to(dev), torch.as_tensor(idx).to(dev)] = torch.as_tensor(val).to(dev)
    tmpl = torch.zeros(A, I, device=dev)
    rows = np.repeat(np.arange(A), np.diff(att.template_rowptr))
    tmpl[torch.as_tensor(rows).to(dev), torch.as_tensor(att.template_cols).to(dev)] = torch.as_tensor(att.template_vals).to(dev)
    l0, l1 = nn.Linear(I, 125).to(dev), nn.Linear(125, I).to(dev)
    minb = torch.ones(I, device=dev, requires_grad=True)
    ilen = torch.ones(I, 3, device=dev, requires_grad=True)
    D = nn.Sequential(nn.Linear(I, 512), nn.ReLU(), nn.Linear(512, 128), nn.ReLU(), nn.Linear(128, 1), nn.Sigmoid()).to(dev)
    g_opt = torch.optim.Adam(list(l0.parameters()) + list(l1.parameters()) + [minb, ilen], lr=att.lr_g)
    d_opt = torch.optim.Adam(D.parameters(), lr=att.lr_d)

    class Heavi(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.save_for_backward(x)
            return (x > 0).float()

        @staticmethod
        def backward(ctx, dy):
            return dy * (1 - torch.tanh(ctx.saved_tensors[0]) ** 2)

    def G(x):
        a = torch.tanh(l1(torch.relu(l0(nn.functional.normalize(x))))) * 2.5 + 2.5
        b = [minb]
        for k in range(3):
            b.append(b[-1] + torch.relu(ilen[:, k]) + 1e-4)
        dist = []
        for c in range(5):
            p = torch.ones_like(a)
            for k in range(4):
                p = p * Heavi.apply((1.0 if k < c else -1.0) * (a - b[k]))
            dist.append(p)
        dist = torch.stack(dist, 2)
        return dist, (dist @ torch.arange(1.0, 6.0, device=dev)) * (x > 0)

    def pretrain_epoch():
        perm = np.random.permutation(U)
        for b in range((U + bs - 1) // bs):
            x = X[torch.as_tensor(perm[b * bs:(b + 1) * bs]).to(dev)]
            dist, _ = G(x)
            lab = x.flatten().long()
            loss = nn.functional.cross_entropy(dist.reshape(-1, 5)[lab > 0], lab[lab > 0] - 1)
            g_opt.zero_grad()
            loss.backward()
            g_opt.step()

    def d_epoch():
        with torch.no_grad():
            fake = G(tmpl)[1]
        perm = np.random.permutation(U)
        for b in range((U + bs - 1) // bs):
            real = X[torch.as_tensor(perm[b * bs:(b + 1) * bs][:A]).to(dev)]
            pr, pf = D(real), D(fake)
            loss = nn.functional.binary_cross_entropy(pr, torch.ones_like(pr)) + nn.functional.binary_cross_entropy(pf, torch.zeros_like(pf))
            d_opt.zero_grad()
            loss.backward()
            d_opt.step()

    def adv():
        p = D(G(tmpl)[1])
        loss = nn.functional.binary_cross_entropy(p, torch.ones_like(p))
        g_opt.zero_grad()
        loss.backward()
        g_opt.step()

    out = []
    for fn in (pretrain_epoch, d_epoch, adv):
        fn()                                    # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def child(shape, fits):
    import numpy as np
    import torch

    from recad_amd import model

    dev = torch.device("cuda:0")
    ds = _data(shape, dev)
    np.random.seed(2)
    torch.manual_seed(2)
    att = model.from_config("attacker", "aushplus", device=dev).I(dataset=ds)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    att.pretrain_G(), att.train_D(), att.train_G_adv(), att.train_G_attack([0])       # warm-up of every path
    t_pg, _ = timed(att.pretrain_G)
    t_d, _ = timed(att.train_D)
    t_adv, _ = timed(att.train_G_adv)
    t_fit, _ = timed(lambda: [att.train_G_attack([0]) for _ in range(fits)])
    t_fit /= fits
    E, Gd, Gg, S = att.pretrain_epoch_g, att.epoch_gan_d, att.epoch_gan_g, att.epoch_surrogate
    res = {"shape": shape, "n_users": att.n_users, "n_items": att.n_items, "fake_entries": att.n_fake,
           "pretrain_G_epoch_s": t_pg, "train_D_epoch_s": t_d, "train_G_adv_s": t_adv, "surrogate_fit_s": t_fit,
           "first_step_pretrain_s": E * (t_pg + t_d), "phase2_s": Gd * t_d, "phase3_s": Gg * t_adv, "phase4_s": S * t_fit,
           "train_step_s": Gd * t_d + Gg * t_adv + S * t_fit}
    res["phases_1_3_below_phase_4"] = bool(res["first_step_pretrain_s"] + res["phase2_s"] + res["phase3_s"] < res["phase4_s"])
    dpg, dd, dadv = dense_phases_s(att, dev)
    res.update({"dense_pretrain_G_epoch_s": dpg, "dense_train_D_epoch_s": dd, "dense_train_G_adv_s": dadv})
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,yelp")
    ap.add_argument("--fits", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.fits)
    lines = []
    for shape in args.shapes.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--fits", str(args.fits)], capture_output=True,
                               text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{shape}: timed out after {args.timeout} s", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(p.stderr[-2000:], file=sys.stderr)
            return p.returncode            # nothing more is started on the GPU after a failure
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
