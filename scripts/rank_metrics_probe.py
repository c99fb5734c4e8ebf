"""Cost of the held-out ranking metrics at the ml1m shape (5 893 eligible users x top-100): rk_rank_metrics alone (a hipGraph of 50
calls, replayed) and an EvalSession replay with and without quality=, alternating, device events around 200 replays each.
usage: python3 scripts/rank_metrics_probe.py"""
import sys
import numpy as np, torch
sys.path.insert(0, '.')
from recad_amd import _lib, dataset, model, synth
from recad_amd.evaluate import EvalSession, eligible_users, rank_metrics

dev = torch.device('cuda:0')
d = synth.make("ml1m")
ds = dataset.from_config("implicit", "ml1m", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], device=dev, graph_source="train")
victim = model.from_config("victim", "lightgcn", latent_dim_rec=64).I(dataset=ds).to(dev)
ptr, idx = ds.train_csr_sorted()
targets = np.array([0], dtype=np.int32)
ev = eligible_users(ptr, idx, targets)
t = lambda a: torch.as_tensor(a, dtype=torch.int32, device=dev)
topks = (10, 20, 50, 100)
gt = tuple(t(a) for a in ds.heldout_csr("test"))
sessions = {"plain": EvalSession(victim, t(ev), t(ptr), t(idx), t(targets), K=100, topks=topks),
            "quality": EvalSession(victim, t(ev), t(ptr), t(idx), t(targets), K=100, topks=topks, quality=gt)}
for s in sessions.values():
    for _ in range(4):
        s.run()
torch.cuda.synchronize()
print(f"{len(ev)} users, {int(gt[1].numel())} held-out items", flush=True)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


for rnd in range(5):
    print("  ".join(f"{name} {timed(s.run, 200):.1f} us" for name, s in sessions.items()), "per evaluation", flush=True)

top = sessions["quality"].top_ids
users = t(ev)
rank_metrics(top, users, *gt, topks, to_host=False)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    for _ in range(50):
        keep = rank_metrics(top, users, *gt, topks, to_host=False)
for rnd in range(5):
    print(f"rk_rank_metrics alone: {timed(g.replay, 20) / 50:.2f} us per call (50 calls per replay)", flush=True)
print(rank_metrics(top, users, *gt, topks))
