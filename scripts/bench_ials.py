"""iALS victim timings (not the driver's bench line): d = 64, alpha = 40, lambda = 10, on the train edges of
recad_amd.synth.make_device("ml1m") with every value 1.0.  One sweep is rk_ials_gram + rk_ials_half_sweep over the users, the same
over the items, and the float64 objective (rk_ials_gram64 + rk_ials_objective); train_step also reads the status words and J back.
Every number is the median of single train_step calls timed by device events after warm calls.

Counted work of a half-sweep: 2 nnz d^2 flops for the rank-n_u updates (the full d x d product; the kernel computes the lower
triangle's tiles only) plus n_rows d^3 / 3 for the Cholesky factorisations; the line gives the two half-sweeps' count over the
whole train_step as a share of the 157.3 TF fp32 MFMA peak.  Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/bench_ials.py --sweeps 3`.

    python scripts/bench_ials.py [--shape ml1m] [--dim 64] [--sweeps 9]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_F32_MFMA_TF = 157.3


class _Mat:
    def __init__(self, csr, n_users, n_items):
        self.csr, self.n_users, self.n_items = csr, n_users, n_items

    def info_describe(self):
        return {"n_users": self.n_users, "n_items": self.n_items, "train_mat": (*self.csr, self.n_items)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml1m")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--sweeps", type=int, default=9)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    from recad_amd import model, synth

    dev = torch.device("cuda:0")
    d = synth.make_device(args.shape, dev)
    ptr, idx = d["train"]
    U, I = d["n_users"], d["n_items"]
    rp, idx = ptr.to(torch.int32).contiguous(), idx.to(torch.int32).contiguous()
    nnz = int(idx.numel())
    val = torch.ones(nnz, dtype=torch.float32, device=dev)
    v = model.from_config("victim", "ials", factor_num=args.dim, seed=1).I(dataset=_Mat((rp, idx, val), U, I)).to(dev)
    losses = [v.train_step()[0] for _ in range(2)]          # warm: the CSR cache, the transpose, the kernels' first launches
    torch.cuda.synchronize()
    times = []
    for _ in range(args.sweeps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        losses.append(v.train_step()[0])
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = statistics.median(times)
    flops = 2 * (2.0 * nnz * args.dim ** 2) + (U + I) * args.dim ** 3 / 3.0
    print(json.dumps({"shape": args.shape, "n_users": U, "n_items": I, "nnz": nnz, "dim": args.dim, "alpha": 40.0, "reg_lambda": 10.0,
                      "sweeps": args.sweeps, "sweep_ms": round(ms, 3), "sweep_ms_min_max": [round(min(times), 3), round(max(times), 3)],
                      "sweep_flops": flops, "tflops_whole_step": round(flops / ms / 1e9, 3),
                      "share_of_f32_mfma_peak_whole_step": round(flops / ms / 1e9 / PEAK_F32_MFMA_TF, 5),
                      "loss_first_last": [losses[0], losses[-1]]}))


if __name__ == "__main__":
    main()
