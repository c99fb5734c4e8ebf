"""Mult-VAE victim timings (not the driver's bench line): rk_mvae_train_epoch at the ml1m shape (5 950 x 3 702) and the yelp shape
(54 632 x 34 474) of recad_amd.synth.make_device with the defaults H = 600, L = 200, B = 500, dropout 0.5, and one evaluation
(score_matrix + rk_topk_rows, K = 100, every user with a train list).  The users of a step are `--steps` * B draws from the users
with a train list, so the rows have the real degrees.

What is timed.  Whole calls by device events after two warm calls, `--reps` of them, reported as median / min / max: a call is the
id check with its one read-back and the steps, so us_per_step is the call over the steps and includes it.  The split per kernel
comes from a separate run under `rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/bench_multvae.py --reps 3
--no-comparator --no-eval`, with nothing else traced in it: the library call has no seam to put an event into.

The comparator runs in the same process on the same card: the same step composed from torch ops -- the batch's rows as a dense
B x I matrix built by index_put, a Bernoulli mask from torch's generator, three nn.Linear-shaped products with tanh, the sample,
log_softmax, autograd and torch.optim.Adam.  It computes the same model with other masks and other noise; it is a timing yardstick,
not a check.

Counted per step, so a reader can see how far a kernel is from a bound: the FLOPs of each product (2 M N K), against 157.3 TF/s
for fp32 MFMA; the row kernel reads each logits row three times and writes it once (16 B I bytes at most, 8 B I if the row stays
in cache between the passes); gW1 reads H floats per kept entry and writes I H (4 H (kept + I) bytes); the sparse layer reads H
floats per stored entry; Adam reads and writes p, m, v and reads g (28 bytes an element).

    python scripts/bench_multvae.py [--shape ml1m|yelp] [--steps 12] [--reps 7] [--no-comparator] [--no-eval] [--out profiles/bench_multvae_mi355x.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, L, B, DROPOUT, CAP, TOTAL, LR, B1, B2, ADAM_EPS, TOPK = 600, 200, 500, 0.5, 0.2, 200000, 1e-3, 0.9, 0.999, 1e-8, 100
PEAK_F32_MFMA_TF = 157.3


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


class _Mat:
    def __init__(self, csr, n_users, n_items):
        self.csr, self.n_users, self.n_items = csr, n_users, n_items

    def info_describe(self):
        return {"n_users": self.n_users, "n_items": self.n_items, "train_mat": (*self.csr, self.n_items)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml1m", choices=("ml1m", "yelp"))
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-comparator", action="store_true")
    ap.add_argument("--no-eval", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_multvae_mi355x.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    from recad_amd import _lib, model, synth

    _lib.require_gpu()
    dev = torch.device("cuda:0")
    data = synth.make_device(args.shape, dev)
    U, I, S = data["n_users"], data["n_items"], args.steps
    ptr, idx = data["train"]
    rp, col = ptr.to(torch.int32).contiguous(), idx.to(torch.int32).contiguous()
    val = torch.ones(col.numel(), dtype=torch.float32, device=dev)
    lens = (rp[1:] - rp[:-1]).long()
    have = torch.nonzero(lens > 0).view(-1)
    gen = torch.Generator(device=dev).manual_seed(1)
    n = S * B
    ids = have[torch.randint(0, have.numel(), (n,), device=dev, generator=gen)].to(torch.int32).contiguous()
    step_nnz = lens[ids.long()].view(S, B).sum(dim=1)
    Lb, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)

    v = model.from_config("victim", "multvae", hidden_dim=H, latent_dim=L, batch_size=B, dropout=DROPOUT, anneal_cap=CAP, total_anneal_steps=TOTAL,
                          lr=LR, seed=1).I(dataset=_Mat((rp, col, val), U, I)).to(dev)
    theta0 = v.theta.data.clone()
    losses = torch.empty(3 * S, dtype=torch.float64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)

    def fresh():
        v.theta.data.copy_(theta0)
        for k in ("exp_avg", "exp_avg_sq"):
            v._adam_slot(v.theta)[k].zero_()

    def epoch():
        desc = v._desc(dev, training=True)
        _lib.check(Lb.rk_mvae_train_epoch(C.byref(desc), P(ids), n, B, 0, 1, P(losses), P(status), s), "rk_mvae_train_epoch")

    fresh()
    v._desc(dev)                                                               # lays the workspace out
    kept = float(step_nnz.float().mean()) * (1.0 - DROPOUT)
    entries = float(step_nnz.float().mean())
    gemms = {"ml (B x 2L x H)": 2.0 * B * 2 * L * H, "pre2 (B x H x L)": 2.0 * B * H * L, "logits (B x I x H)": 2.0 * B * I * H,
             "gW4 (I x H x B)": 2.0 * I * H * B, "dh2 (B x H x I)": 2.0 * B * H * I, "gW3 (H x L x B)": 2.0 * H * L * B,
             "dz (B x L x H)": 2.0 * B * L * H, "gW2 (2L x H x B)": 2.0 * 2 * L * H * B, "dh1 (B x H x 2L)": 2.0 * B * H * 2 * L}
    n_params = int(v.theta.numel())
    out = {"shape": args.shape, "n_users": U, "n_items": I, "hidden": H, "latent": L, "batch": B, "steps": S, "reps": args.reps,
           "n_params": n_params, "workspace_bytes": int(v._ws[1].bytes), "entries_per_step": entries,
           "gemm_flops_per_step": gemms, "gemm_flops_total": sum(gemms.values()),
           "row_kernel_bytes_per_step": [8.0 * B * I, 16.0 * B * I], "gw1_bytes_per_step": 4.0 * H * (kept + I),
           "sparse_layer_bytes_per_step": 4.0 * H * kept, "adam_bytes_per_step": 28.0 * n_params}
    t = _timed(epoch, args.reps)
    out["us_per_step"] = {k: round(x * 1e3 / S, 2) for k, x in t.items()}
    out["tflops_all_gemms_over_the_whole_step"] = round(sum(gemms.values()) / (t["median"] * 1e-3 / S) / 1e12, 2)
    out["losses_last_step"] = [round(float(x), 6) for x in losses[-3:].cpu()]

    if not args.no_comparator:
        lin = lambda o, i: torch.nn.Linear(i, o, device=dev)
        enc1, enc2, dec1, dec2 = lin(H, I), lin(2 * L, H), lin(H, L), lin(I, H)
        params = [p for m in (enc1, enc2, dec1, dec2) for p in m.parameters()]
        opt = torch.optim.Adam(params, lr=LR)
        rows = torch.repeat_interleave(torch.arange(U, device=dev), lens)
        dense = torch.zeros(U, I, device=dev)
        dense[rows, idx.long()] = 1.0                                          # outside the timed window
        idl = ids.long().view(S, B)

        def composed():
            for st in range(S):
                X = dense[idl[st]]
                nrm = X.sum(dim=1, keepdim=True).rsqrt()
                Xin = torch.nn.functional.dropout(X * nrm, DROPOUT, training=True)
                h1 = torch.tanh(enc1(Xin))
                ml = enc2(h1)
                mu, lv = ml[:, :L], ml[:, L:]
                z = mu + torch.randn_like(mu) * torch.exp(0.5 * lv)
                logits = dec2(torch.tanh(dec1(z)))
                nll = -(torch.log_softmax(logits, dim=1) * X).sum(dim=1)
                kl = -0.5 * (1 + lv - mu * mu - lv.exp()).sum(dim=1)
                loss = (nll + CAP * kl).mean()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()

        tc = _timed(composed, max(3, args.reps // 2), warm=1)
        out["composed_reps"] = max(3, args.reps // 2)
        out["composed_us_per_step"] = {k: round(x * 1e3 / S, 2) for k, x in tc.items()}
        out["composed_over_hip"] = round(tc["median"] / t["median"], 3)
        del dense

    if not args.no_eval:
        users = have.to(torch.int32).contiguous()
        ne = int(users.numel())
        chunk = 2048
        scores = torch.empty(chunk * I, dtype=torch.float32, device=dev)
        top_ids, top_scores = torch.empty(ne, TOPK, dtype=torch.int32, device=dev), torch.empty(ne, TOPK, dtype=torch.float32, device=dev)
        tg = torch.zeros(1, dtype=torch.int32, device=dev)
        tscore, trank = torch.empty(ne, 1, dtype=torch.float32, device=dev), torch.empty(ne, 1, dtype=torch.int32, device=dev)

        def evaluate(topk=True):
            for a in range(0, ne, chunk):
                e = min(ne, a + chunk)
                v.score_matrix(users[a:e], scores[:(e - a) * I])
                if topk:
                    _lib.check(Lb.rk_topk_rows(P(scores), e - a, I, P(users[a:e]), P(rp), P(col), TOPK, P(top_ids[a:e]), P(top_scores[a:e]), P(tg), 1,
                                               P(tscore[a:e]), P(trank[a:e]), s), "rk_topk_rows")

        ts, te = _timed(lambda: evaluate(False), args.reps, warm=1), _timed(evaluate, args.reps, warm=1)
        out.update(n_eval_users=ne, eval_chunk=chunk, score_matrix_ms=round(ts["median"], 3), score_and_topk_ms=round(te["median"], 3),
                   score_flops=2.0 * ne * H * (I + 2 * L))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
