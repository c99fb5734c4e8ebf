"""PGA attacker timings (not the driver's bench line): one train_step at the ml1m shape (recad_amd.synth.make_device("ml1m"),
seeded 1..5 ratings), attack_num = 50, filler_num = 36, alpha = 40, lambda = 10, sweeps_s = 2, d = 16 and d = 64.

Two numbers per d, alternated in one process after warm calls, medians of device-event timings around whole steps:
  * train_step of recad_amd.attack.PGA, and in a second pass the time per entry point: every call into the library is bracketed by
    device events (the brackets cost launches, so the whole-step figure comes from the first pass);
  * the same iteration composed from torch ops on the device in fp32, nothing of csrc/pga.hip: one sweep without a graph, one sweep
    under autograd (batched torch.linalg.solve of the d x d systems, the systems formed by dense [rows, I] x [I, d^2] products),
    the masked log-softmax loss, backward to the A x I strengths, the normalised step, and torch.topk for the selection.
The composed form also reports max |grad - grad_device| / max |grad| from the same tables' start, as a check that both compute
the same thing.

    python scripts/bench_pga.py [--shape ml1m] [--dims 16 64] [--reps 5] [--out profiles/bench_pga_mi355x.jsonl]
"""
import argparse
import collections
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Ratings:
    """What attack/_common.train_csr asks of a dataset."""

    def __init__(self, csr, n_users, n_items):
        self.csr, self.n_users, self.n_items = csr, n_users, n_items

    def rating_csr(self, split):
        return self.csr


class _Timed:
    """The library with every entry bracketed by device events."""

    def __init__(self, lib, torch):
        self.lib, self.torch, self.events = lib, torch, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("rk_") or name == "rk_last_error":
            return fn

        def call(*a):
            e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self.events.append((name, e0, e1))
            return rc

        return call

    def totals(self):
        self.torch.cuda.synchronize()
        out = collections.OrderedDict()
        for name, e0, e1 in self.events:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        self.events = []
        return out


def composed_step(torch, st, R, Y, n_sweeps):
    """One iteration from torch ops: returns (loss, grad, new R, new profile columns, Y+)."""
    W, Cp, rated, elig, inv, target, wbar, lam, lr, F = (st[k] for k in ("W", "Cp", "rated", "elig", "inv", "target", "wbar", "lam", "lr", "F"))
    d = Y.shape[1]
    eye = torch.eye(d, device=Y.device)

    def half(Wm, Cm, T):
        """rows solved from the other side's table T: A = T^T T + lam I + sum_e w t t^T, b = sum_e c t"""
        TT = (T[:, :, None] * T[:, None, :]).reshape(T.shape[0], d * d)
        Am = (T.T @ T + lam * eye)[None] + (Wm @ TT).reshape(-1, d, d)
        return torch.linalg.solve(Am, (Cm @ T)[:, :, None])[:, :, 0]

    mask = torch.zeros_like(R)
    mask.scatter_(1, torch.topk(R.masked_fill(st["tmask"], -1.0), F, dim=1).indices, 1.0)
    mask[:, target] = 1.0
    with torch.no_grad():
        for _ in range(n_sweeps - 1):
            X = half(torch.cat([W, wbar * mask]), torch.cat([Cp, (1.0 + wbar) * mask]), Y)
            Y = half(torch.cat([W, wbar * mask]).T.contiguous(), torch.cat([Cp, (1.0 + wbar) * mask]).T.contiguous(), X)
        Xr = half(W, Cp, Y)
    r = mask.clone().requires_grad_(True)
    Xf = half(wbar * r, (1.0 + wbar) * r, Y)
    X = torch.cat([Xr, Xf])
    Yp = half(torch.cat([W, wbar * r]).T, torch.cat([Cp, (1.0 + wbar) * r]).T, X)
    S = Xr @ Yp.T
    lse = torch.logsumexp(S.masked_fill(rated, float("-inf")), dim=1)
    loss = ((lse - S[:, target]) * elig).sum() * inv
    (grad,) = torch.autograd.grad(loss, r)
    m = grad.abs().max()
    Rn = torch.clamp(R - lr * grad / m, 0.0, 1.0) if float(m) > 0 else R
    Rn[:, target] = 1.0
    cols = torch.topk(Rn.masked_fill(st["tmask"], -1.0), F, dim=1).indices
    return loss.detach(), grad, Rn, cols, Yp.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml1m")
    ap.add_argument("--dims", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_pga_mi355x.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from recad_amd import _lib, model, synth

    dev = torch.device("cuda:0")
    data = synth.make_device(args.shape, dev)
    ptr, idx = (t.cpu().numpy() for t in data["train"])
    U, I = data["n_users"], data["n_items"]
    val = np.clip(np.round(np.random.default_rng(7).normal(3.6, 1.1, len(idx))), 1, 5).astype(np.float32)
    ds = _Ratings((ptr.astype(np.int64), idx.astype(np.int32), val), U, I)
    target, A, F, alpha, lam, lr = 0, 50, 36, 40.0, 10.0, 0.25
    rows = np.repeat(np.arange(U), np.diff(ptr))
    lines = []
    for d in args.dims:
        def fresh():
            np.random.seed(3)
            return model.from_config("attacker", "pga", device=dev, attack_num=A, filler_num=F, factor_num_s=d, alpha_s=alpha,
                                     reg_lambda_s=lam, lr=lr, init_sweeps_s=2, sweeps_s=2, seed_s=1).I(dataset=ds)

        att = fresh()
        # the composed form's dense data, and its start: the device attacker's strengths and seeded item table
        Q = torch.zeros(U, I, device=dev)
        Q[torch.as_tensor(rows, device=dev), torch.as_tensor(idx.astype(np.int64), device=dev)] = torch.as_tensor(val, device=dev)
        elig = (Q[:, target] == 0).float()
        tmask = torch.zeros(A, I, dtype=torch.bool, device=dev)
        tmask[:, target] = True
        st = {"W": alpha * Q, "Cp": torch.where(Q > 0, 1.0 + alpha * Q, torch.zeros_like(Q)), "rated": Q > 0, "elig": elig,
              "inv": 1.0 / float(elig.sum()), "target": target, "wbar": alpha * 5.0, "lam": lam, "lr": lr, "F": F, "tmask": tmask}
        R0, Y0 = att._R.clone(), att._Y.clone()
        loss_c, grad_c, _, _, _ = composed_step(torch, st, R0, Y0, 2)
        (loss_d,) = att.train_step(target_id_list=[target])
        gd = torch.as_tensor(att.last_gradient(), device=dev)
        agree = float((grad_c - gd).abs().max() / gd.abs().max())
        state = {"R": R0, "Y": Y0}
        t_dev, t_comp = [], []
        for rep in range(args.reps + 2):                     # two warm rounds of each, then alternating
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            att.train_step(target_id_list=[target])
            e[1].record()
            e[2].record()
            _, _, state["R"], _, state["Y"] = composed_step(torch, st, state["R"], state["Y"], 2)
            e[3].record()
            torch.cuda.synchronize()
            if rep >= 2:
                t_dev.append(e[0].elapsed_time(e[1]))
                t_comp.append(e[2].elapsed_time(e[3]))
        real = _lib.lib()
        timed = _Timed(real, torch)
        per = []
        try:
            _lib._lib = timed
            for _ in range(args.reps):
                att.train_step(target_id_list=[target])
                per.append(timed.totals())
        finally:
            _lib._lib = real
        entries = {k: round(statistics.median(p[k] for p in per), 4) for k in per[0]}
        total = sum(entries.values())
        line = {"shape": args.shape, "n_users": U, "n_items": I, "nnz": int(len(idx)), "attack_num": A, "filler_num": F, "dim": d,
                "alpha": alpha, "reg_lambda": lam, "sweeps_s": 2, "reps": args.reps,
                "train_step_ms": {"median": round(statistics.median(t_dev), 3), "min": round(min(t_dev), 3), "max": round(max(t_dev), 3)},
                "composed_torch_ms": {"median": round(statistics.median(t_comp), 3), "min": round(min(t_comp), 3), "max": round(max(t_comp), 3)},
                "composed_over_train_step": round(statistics.median(t_comp) / statistics.median(t_dev), 3),
                "entry_ms": entries, "entry_share": {k: round(v / total, 4) for k, v in entries.items()},
                "loss_device_vs_composed": [loss_d, float(loss_c)], "grad_max_rel_difference": agree}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del Q, st, att
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
