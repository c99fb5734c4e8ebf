#!/usr/bin/env python3
"""Generate the golden input/output vectors under tests/golden/ by IMPORTING the
reference (gusye1234/recad v0.0.2, a checkout passed as --reference).

This script is the provenance of every ``*.npz`` in this directory.  It is run
by hand on a machine that has a checkout of the reference;
nothing under ``tests/`` or the product imports it.  It copies no reference
source: it drives the reference's public objects

    recad.dataset.from_config / recad.model.from_config / victim.train_step /
    victim.forward / Normal.user_item_model_generate

and records inputs (graph, tables, the exact minibatches the reference's own
sampler produced) and outputs (per-step loss, step-1 gradients, tables, scores,
top-K lists, HR@K rows).

Usage:
    python tests/golden/make_golden.py --reference PATH [--scratch /tmp/recad_golden_scratch]

Determinism: the reference is bit-reproducible only with 1 intra-op thread
(SURVEY.md section 8c), so we pin ``torch.set_num_threads(1)``.
"""
import argparse
import os
import shutil
import sys
import zipfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))


def seeded_table(seed, rows, dim, std):
    """Initial tables the tests can regenerate without storing them (PCG64)."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, dim), dtype=np.float32) * np.float32(std)).astype(np.float32)


def seeded_uniform(seed, rows, dim, lo, hi):
    rng = np.random.default_rng(seed)
    return (rng.random((rows, dim), dtype=np.float32) * np.float32(hi - lo) + np.float32(lo)).astype(np.float32)


def dict_to_csr(d, n_rows):
    ptr = np.zeros(n_rows + 1, dtype=np.int64)
    for u, items in d.items():
        ptr[int(u) + 1] = len(items)
    ptr = np.cumsum(ptr)
    idx = np.zeros(ptr[-1], dtype=np.int32)
    for u, items in d.items():
        idx[ptr[int(u)]:ptr[int(u) + 1]] = np.asarray(items, dtype=np.int32)
    return ptr.astype(np.int32), idx


class OneBatch:
    """Stand-in for dataset.generate_batch that replays a fixed list of batches."""

    def __init__(self, batches):
        self.batches = batches

    def __call__(self, **kw):
        for b in self.batches:
            yield b


def run_per_step(model, dataset, batches):
    """Call the reference's train_step once per recorded batch -> exact per-step loss."""
    import torch

    orig = dataset.generate_batch
    losses = []
    snaps = {}
    try:
        for i, b in enumerate(batches):
            dataset.generate_batch = OneBatch([b])
            (loss,) = model.train_step(progress_bar=None)
            losses.append(loss)
            if i == 0:
                snaps["grad1"] = {n: p.grad.detach().clone().numpy() for n, p in model.named_parameters() if p.grad is not None}
                snaps["after1"] = {n: p.detach().clone().numpy() for n, p in model.named_parameters()}
    finally:
        dataset.generate_batch = orig
    snaps["after_all"] = {n: p.detach().clone().numpy() for n, p in model.named_parameters()}
    return np.asarray(losses, dtype=np.float64), snaps


def eval_rows(recad, model, dataset, target_ids, topks, max_users=None):
    """Reference evaluation for ONE model: candidate dict exactly as
    Normal.normal_evaluate builds it, rows from Normal.user_item_model_generate,
    plus per-user scores so the tests can compare top-K lists."""
    import torch

    info = dataset.info_describe()
    train_dict, n_items = info["train_dict"], info["n_items"]
    full = set(range(n_items))
    cand = {}
    for k, v in train_dict.items():
        s = set(v)
        if any(t in s for t in target_ids):
            continue
        cand[k] = list(full - s)
    if max_users is not None:   # big towers: the reference's per-user loop is evaluated on the first users only
        cand = {k: cand[k] for k in sorted(cand)[:max_users]}
    wf = object.__new__(recad.workflow.Normal)  # only the bound method is needed
    rows = recad.workflow.Normal.user_item_model_generate(wf, model, cand, topks, target_ids, torch.device("cpu"))
    # per-user top-100 by the reference's own forward; stable sort, ties reported
    users = np.array(sorted(cand.keys()), dtype=np.int32)
    top_ids = np.full((len(users), 100), -1, dtype=np.int32)
    top_scores = np.zeros((len(users), 100), dtype=np.float32)
    min_gap = np.zeros(len(users), dtype=np.float32)
    with torch.no_grad():
        for r, u in enumerate(users):
            iids = torch.tensor(cand[int(u)], dtype=torch.int64)
            s = model(torch.full_like(iids, int(u)), iids).numpy()
            order = np.lexsort((iids.numpy(), -s.astype(np.float64)))  # score desc, id asc
            k = min(100, len(order))
            top_ids[r, :k] = iids.numpy()[order[:k]]
            top_scores[r, :k] = s[order[:k]]
            kk = min(101, len(order))
            ss = s[order[:kk]].astype(np.float64)
            gaps = (ss[:-1] - ss[1:]) / np.maximum(np.abs(ss[:-1]), 1e-30)
            min_gap[r] = gaps.min() if len(gaps) else 1.0
    return rows, users, top_ids, top_scores, min_gap


def golden_lightgcn(recad, torch, name, dim, layers, tag, max_steps=None, row_stride=1, eval_stride=1,
                    graph_from_train=False, epochs=1):
    torch.manual_seed(2023)
    np.random.seed(2023)
    ds = recad.dataset.from_config("implicit", name, need_graph=True, sample="pairwise", download=False)
    if graph_from_train:
        # The reference builds its graph from whatever read_data() saw LAST (the test
        # split, implicit.py:173-192,206-209).  Passing the train edges as test_dict
        # makes the reference itself build the *intended* train graph.
        td = ds.info_describe()["train_dict"]
        ds = ds.reset(train_dict=td, test_dict=td)
    info = ds.info_describe()
    U, I = info["n_users"], info["n_items"]
    g = info["graph"]
    model = recad.model.from_config("victim", "lightgcn", latent_dim_rec=dim, lightGCN_n_layers=layers).I(dataset=ds)
    ref_init_user = model.embedding_user.weight.detach().clone().numpy()
    ref_init_item = model.embedding_item.weight.detach().clone().numpy()
    # replace with tables the tests can regenerate
    model.embedding_user.weight.data.copy_(torch.from_numpy(seeded_table(11, U, dim, 0.1)))
    model.embedding_item.weight.data.copy_(torch.from_numpy(seeded_table(12, I, dim, 0.1)))

    batches = []
    for _ in range(epochs):
        batches += list(ds.generate_batch())
    if max_steps:
        batches = batches[:max_steps]
    with torch.no_grad():
        lu, li = model.computer()
        light0 = torch.cat([lu, li]).numpy()
    losses, snaps = run_per_step(model, ds, batches)
    B = max(len(b["users"]) for b in batches)
    bt = np.full((len(batches), 3, B), -1, dtype=np.int32)
    blen = np.zeros(len(batches), dtype=np.int32)
    for s, b in enumerate(batches):
        n = len(b["users"])
        blen[s] = n
        bt[s, 0, :n] = b["users"].numpy()
        bt[s, 1, :n] = b["positive_items"].numpy()
        bt[s, 2, :n] = b["negative_items"].numpy()
    target_ids, topks = [0], [10, 20, 50, 100]
    rows, users, top_ids, top_scores, min_gap = eval_rows(recad, model, ds, target_ids, topks)
    tptr, tidx = dict_to_csr(info["train_dict"], U)
    tsptr, tsidx = dict_to_csr(info["test_dict"], U)
    rs = slice(None, None, row_stride)
    es = slice(None, None, eval_stride)
    out = dict(
        n_users=U, n_items=I, dim=dim, layers=layers, lam=1e-4, lr=1e-3, row_stride=row_stride, eval_stride=eval_stride,
        graph_row=g.indices()[0].numpy().astype(np.int32), graph_col=g.indices()[1].numpy().astype(np.int32),
        graph_val=g.values().numpy(),
        train_ptr=tptr, train_idx=tidx, test_ptr=tsptr, test_idx=tsidx,
        traindata_size=ds.traindataSize,
        batches=bt, batch_len=blen, losses=losses,
        light0=light0[rs],
        grad1_user=snaps["grad1"]["embedding_user.weight"][rs], grad1_item=snaps["grad1"]["embedding_item.weight"][rs],
        after1_user=snaps["after1"]["embedding_user.weight"][rs], after1_item=snaps["after1"]["embedding_item.weight"][rs],
        final_user=snaps["after_all"]["embedding_user.weight"][rs], final_item=snaps["after_all"]["embedding_item.weight"][rs],
        final_user_sum=snaps["after_all"]["embedding_user.weight"].astype(np.float64).sum(0),
        final_item_sum=snaps["after_all"]["embedding_item.weight"].astype(np.float64).sum(0),
        eval_rows=rows, eval_users=users, top_ids=top_ids[es], top_scores=top_scores[es], top_min_gap=min_gap,
        target_ids=np.asarray(target_ids, dtype=np.int32), topks=np.asarray(topks, dtype=np.int32),
    )
    if row_stride == 1:
        out["ref_init_user"] = ref_init_user
        out["ref_init_item"] = ref_init_item
    else:
        out["ref_init_user"] = ref_init_user[rs]
        out["ref_init_item"] = ref_init_item[rs]
    np.savez_compressed(os.path.join(OUT, f"lightgcn_{tag}.npz"), **out)
    print(f"lightgcn_{tag}: U={U} I={I} nnz={g._nnz()} steps={len(batches)} loss0={losses[0]:.6f} lossN={losses[-1]:.6f}")


def pointwise_batches(ds, max_steps):
    batches = []
    for b in ds.generate_batch():
        batches.append(b)
        if max_steps and len(batches) >= max_steps:
            break
    return batches


def pack_pointwise(batches):
    B = max(len(b["users"]) for b in batches)
    bt = np.full((len(batches), 3, B), -1, dtype=np.int32)
    blen = np.zeros(len(batches), dtype=np.int32)
    for s, b in enumerate(batches):
        n = len(b["users"])
        blen[s] = n
        bt[s, 0, :n] = b["users"].numpy()
        bt[s, 1, :n] = b["items"].numpy()
        bt[s, 2, :n] = b["labels"].numpy()
    return bt, blen


def golden_mf(recad, torch, name, dim, tag, max_steps=None, row_stride=1, eval_stride=1):
    torch.manual_seed(2023)
    np.random.seed(2023)
    ds = recad.dataset.from_config("implicit", name, need_graph=False, sample="pointwise", download=False)
    info = ds.info_describe()
    U, I = info["n_users"], info["n_items"]
    model = recad.model.from_config("victim", "mf", embedding_size=dim).I(dataset=ds)
    ref_init = {n: p.detach().clone().numpy() for n, p in model.named_parameters()}
    model.user_emb.weight.data.copy_(torch.from_numpy(seeded_uniform(21, U, dim, 0, 0.005)))
    model.item_emb.weight.data.copy_(torch.from_numpy(seeded_uniform(22, I, dim, 0, 0.005)))
    model.user_bias.weight.data.copy_(torch.from_numpy(seeded_uniform(23, U, 1, -0.01, 0.01)))
    model.item_bias.weight.data.copy_(torch.from_numpy(seeded_uniform(24, I, 1, -0.01, 0.01)))
    batches = pointwise_batches(ds, max_steps)
    losses, snaps = run_per_step(model, ds, batches)
    bt, blen = pack_pointwise(batches)
    target_ids, topks = [0], [10, 20, 50, 100]
    rows, users, top_ids, top_scores, min_gap = eval_rows(recad, model, ds, target_ids, topks)
    tptr, tidx = dict_to_csr(info["train_dict"], U)
    rs = slice(None, None, row_stride)
    es = slice(None, None, eval_stride)
    out = dict(
        n_users=U, n_items=I, dim=dim, lr=1e-3, mean=float(model.mean.item()), row_stride=row_stride, eval_stride=eval_stride,
        train_ptr=tptr, train_idx=tidx, batches=bt, batch_len=blen, losses=losses,
        target_ids=np.asarray(target_ids, dtype=np.int32), topks=np.asarray(topks, dtype=np.int32),
        eval_rows=rows, eval_users=users, top_ids=top_ids[es], top_scores=top_scores[es], top_min_gap=min_gap,
    )
    for k in ("user_emb.weight", "item_emb.weight", "user_bias.weight", "item_bias.weight"):
        kk = k.replace(".weight", "")
        out[f"grad1_{kk}"] = snaps["grad1"][k][rs]
        out[f"after1_{kk}"] = snaps["after1"][k][rs]
        out[f"final_{kk}"] = snaps["after_all"][k][rs]
        out[f"ref_init_{kk}"] = ref_init[k][rs]
    np.savez_compressed(os.path.join(OUT, f"mf_{tag}.npz"), **out)
    print(f"mf_{tag}: U={U} I={I} steps={len(batches)} loss0={losses[0]:.6f} lossN={losses[-1]:.6f}")


def golden_ncf(recad, torch, name, factor, layers, tag, max_steps=None, row_stride=1, eval_stride=1, dense_stride=1,
               eval_max_users=None):
    torch.manual_seed(2023)
    np.random.seed(2023)
    ds = recad.dataset.from_config("implicit", name, need_graph=False, sample="pointwise", download=False)
    info = ds.info_describe()
    U, I = info["n_users"], info["n_items"]
    model = recad.model.from_config("victim", "ncf", factor_num=factor, num_layers=layers).I(dataset=ds)
    E = factor * 2 ** (layers - 1)
    ref_init = {n: p.detach().clone().numpy() for n, p in model.named_parameters()}
    model.embed_user_GMF.weight.data.copy_(torch.from_numpy(seeded_table(31, U, factor, 0.01)))
    model.embed_item_GMF.weight.data.copy_(torch.from_numpy(seeded_table(32, I, factor, 0.01)))
    model.embed_user_MLP.weight.data.copy_(torch.from_numpy(seeded_table(33, U, E, 0.01)))
    model.embed_item_MLP.weight.data.copy_(torch.from_numpy(seeded_table(34, I, E, 0.01)))
    # dense weights: regenerable too (xavier-scale uniform from PCG64), biases stay 0 as the reference sets them
    dense_names = [n for n, p in model.named_parameters() if not n.startswith("embed_") and p.dim() == 2]
    for j, n in enumerate(dense_names):
        p = dict(model.named_parameters())[n]
        a = float(np.sqrt(6.0 / (p.shape[0] + p.shape[1])))
        p.data.copy_(torch.from_numpy(seeded_uniform(40 + j, p.shape[0], p.shape[1], -a, a)))
    batches = pointwise_batches(ds, max_steps)
    with torch.no_grad():
        b0 = batches[0]
        pred0 = model(b0["users"], b0["items"]).numpy()
    losses, snaps = run_per_step(model, ds, batches)
    bt, blen = pack_pointwise(batches)
    target_ids, topks = [0], [10, 20, 50, 100]
    rows, users, top_ids, top_scores, min_gap = eval_rows(recad, model, ds, target_ids, topks, max_users=eval_max_users)
    tptr, tidx = dict_to_csr(info["train_dict"], U)
    rs = slice(None, None, row_stride)
    es = slice(None, None, eval_stride)
    out = dict(
        n_users=U, n_items=I, factor=factor, layers=layers, lr=1e-3, row_stride=row_stride, eval_stride=eval_stride,
        train_ptr=tptr, train_idx=tidx, batches=bt, batch_len=blen, losses=losses, pred0=pred0,
        target_ids=np.asarray(target_ids, dtype=np.int32), topks=np.asarray(topks, dtype=np.int32),
        eval_rows=rows, eval_users=users, top_ids=top_ids[es], top_scores=top_scores[es], top_min_gap=min_gap,
    )
    out["dense_names"] = np.asarray(dense_names)
    out["dense_stride"] = dense_stride
    for n in snaps["after_all"]:
        emb = n.startswith("embed_")
        pick = (lambda a: a[rs]) if emb else (lambda a: a.reshape(-1)[::dense_stride])
        if n in snaps["grad1"]:
            out["grad1_" + n] = pick(snaps["grad1"][n])
        out["after1_" + n] = pick(snaps["after1"][n])
        out["final_" + n] = pick(snaps["after_all"][n])
        out["ref_init_" + n] = pick(ref_init[n])[:4096]
    np.savez_compressed(os.path.join(OUT, f"ncf_{tag}.npz"), **out)
    print(f"ncf_{tag}: U={U} I={I} E={E} steps={len(batches)} loss0={losses[0]:.6f} lossN={losses[-1]:.6f}")


def golden_ncf_init_eval(recad, torch, name, factor, layers, tag, eval_max_users, full_score_users=8):
    """The reference's evaluation (Normal.user_item_model_generate, recad/workflow/normal.py:57-93, through
    recad/model/victim/ncf.py:112-131) of the UNTRAINED victim at the seeded initial parameters the tests regenerate
    (tests/_golden.py ncf_init): pins the forward / scoring / top-K path at factor 256 with NO training history -- no ReLU gate
    decided by an earlier step's rounding -- in front of it (round-5 review, next #2).  The scores are recorded from the
    reference's own forward calls inside user_item_model_generate (a recording wrapper around model.forward: one pass)."""
    torch.manual_seed(2023)
    np.random.seed(2023)
    ds = recad.dataset.from_config("implicit", name, need_graph=False, sample="pointwise", download=False)
    info = ds.info_describe()
    U, I = info["n_users"], info["n_items"]
    model = recad.model.from_config("victim", "ncf", factor_num=factor, num_layers=layers).I(dataset=ds)
    E = factor * 2 ** (layers - 1)
    model.embed_user_GMF.weight.data.copy_(torch.from_numpy(seeded_table(31, U, factor, 0.01)))
    model.embed_item_GMF.weight.data.copy_(torch.from_numpy(seeded_table(32, I, factor, 0.01)))
    model.embed_user_MLP.weight.data.copy_(torch.from_numpy(seeded_table(33, U, E, 0.01)))
    model.embed_item_MLP.weight.data.copy_(torch.from_numpy(seeded_table(34, I, E, 0.01)))
    dense_names = [n for n, p in model.named_parameters() if not n.startswith("embed_") and p.dim() == 2]
    for j, n in enumerate(dense_names):
        p = dict(model.named_parameters())[n]
        a = float(np.sqrt(6.0 / (p.shape[0] + p.shape[1])))
        p.data.copy_(torch.from_numpy(seeded_uniform(40 + j, p.shape[0], p.shape[1], -a, a)))
    for n, p in model.named_parameters():    # (the reference zeroes its biases: ncf.py:60-77; stated here, asserted by the tests' init)
        if p.dim() == 1:
            assert float(p.abs().max()) == 0.0, n
    target_ids, topks = [0], [10, 20, 50, 100]
    train_dict = info["train_dict"]
    full = set(range(I))
    cand = {}
    for k, v in train_dict.items():
        s_ = set(v)
        if any(t in s_ for t in target_ids):
            continue
        cand[k] = list(full - s_)
    cand = {k: cand[k] for k in sorted(cand)[:eval_max_users]}
    calls, memo = [], {}
    orig_forward = model.forward

    def recording_forward(users, items):
        # records every forward call of the reference's evaluation loop; a repeated call for the same user with the same items
        # (the extra-target passes below) returns the recorded output instead of recomputing 5 600 towers
        u = int(users[0])
        if u in memo and np.array_equal(memo[u][0], items.numpy()):
            return torch.from_numpy(memo[u][1].copy())
        out = orig_forward(users, items)
        memo[u] = (items.numpy().copy(), out.detach().numpy().copy())
        calls.append((u, memo[u][0], memo[u][1]))
        return out

    model.forward = recording_forward
    wf = object.__new__(recad.workflow.Normal)
    rows0 = recad.workflow.Normal.user_item_model_generate(wf, model, cand, topks, target_ids, torch.device("cpu"))
    users = np.array(sorted(cand.keys()), dtype=np.int32)
    assert [c[0] for c in calls] == users.tolist()
    # an untrained victim ranks item 0 nowhere near anybody's top-100 (all hit flags 0): three more targets, chosen among the items
    # NONE of these users rated (so the candidate lists -- and the recorded forward calls -- stay what they are) as the ones inside the
    # most users' top-50, evaluated by the reference's own loop one target at a time (its row indexing handles one target: normal.py:81-92)
    common = full.copy()
    for k in cand:
        common &= set(cand[k])
    common.discard(0)
    common = np.array(sorted(common), dtype=np.int64)
    in_top50 = np.zeros(I, dtype=np.int64)
    for u, iids, sc in calls:
        order = np.lexsort((iids, -sc.astype(np.float64)))
        in_top50[iids[order[:50]]] += 1
    extra = common[np.argsort(-in_top50[common], kind="stable")[:3]]
    target_ids = [0] + [int(t) for t in extra]
    rows = np.stack([rows0] + [recad.workflow.Normal.user_item_model_generate(wf, model, cand, topks, [int(t)], torch.device("cpu")) for t in extra])
    model.forward = orig_forward
    assert len(calls) == len(users), "the extra-target passes must have been served from the recorded calls"
    top_ids = np.full((len(users), 100), -1, dtype=np.int32)
    top_scores = np.zeros((len(users), 100), dtype=np.float32)
    min_gap = np.zeros(len(users), dtype=np.float32)
    scores_full = np.full((min(full_score_users, len(users)), I), np.nan, dtype=np.float32)   # NaN = a seen item (not scored)
    for r, (u, iids, sc) in enumerate(calls):
        order = np.lexsort((iids, -sc.astype(np.float64)))
        k = min(100, len(order))
        top_ids[r, :k] = iids[order[:k]]
        top_scores[r, :k] = sc[order[:k]]
        ss = sc[order[: min(101, len(order))]].astype(np.float64)
        gaps = (ss[:-1] - ss[1:]) / np.maximum(np.abs(ss[:-1]), 1e-30)
        min_gap[r] = gaps.min() if len(gaps) else 1.0
        if r < scores_full.shape[0]:
            scores_full[r, iids] = sc
    tptr, tidx = dict_to_csr(train_dict, U)
    np.savez_compressed(
        os.path.join(OUT, f"ncf_{tag}_init_eval.npz"),
        n_users=U, n_items=I, factor=factor, layers=layers, eval_stride=1, train_ptr=tptr, train_idx=tidx,
        dense_names=np.asarray(dense_names), target_ids=np.asarray(target_ids, dtype=np.int32), topks=np.asarray(topks, dtype=np.int32),
        eval_rows=rows, eval_users=users, top_ids=top_ids, top_scores=top_scores, top_min_gap=min_gap, scores_full=scores_full,
    )
    print(f"ncf_{tag}_init_eval: U={U} I={I} E={E} users={len(users)} targets={target_ids} hr={rows[:, :, 2:].mean(1).tolist()} "
          f"min_gap>{2e-6}: {(min_gap > 2e-6).sum()}")


def golden_graph_inject(recad, torch, name, tag):
    """Graph before/after inject_data: the normalised adjacency the
    reference builds for a poisoned dataset, for the build's own graph builder."""
    np.random.seed(7)
    ds = recad.dataset.from_config("implicit", name, need_graph=True, sample="pairwise", download=False)
    info = ds.info_describe()
    U, I = info["n_users"], info["n_items"]
    rng = np.random.default_rng(5)
    fake = np.zeros((50, I), dtype=np.float32)
    for r in range(50):
        cols = rng.choice(I, size=36, replace=False)
        fake[r, cols] = rng.integers(1, 6, size=36)
        fake[r, 0] = 5.0
    ds2 = ds.inject_data("explicit", fake, filter_num=4)
    i2 = ds2.info_describe()
    g2 = i2["graph"]
    tptr, tidx = dict_to_csr(i2["train_dict"], i2["n_users"])
    np.savez_compressed(
        os.path.join(OUT, f"inject_{tag}.npz"),
        n_users=U, n_items=I, fake=fake, n_users_after=i2["n_users"], n_items_after=i2["n_items"],
        train_ptr_after=tptr, train_idx_after=tidx, traindata_size_after=ds2.traindataSize,
        graph_row=g2.indices()[0].numpy().astype(np.int32), graph_col=g2.indices()[1].numpy().astype(np.int32),
        graph_val=g2.values().numpy(),
    )
    print(f"inject_{tag}: U {U}->{i2['n_users']} nnz_after={g2._nnz()} train_after={ds2.traindataSize}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (gusye1234/recad v0.0.2): its recad/ and data/")
    ap.add_argument("--scratch", default="/tmp/recad_golden_scratch")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    ref_root = os.path.abspath(args.reference)
    os.makedirs(os.path.join(args.scratch, "data"), exist_ok=True)
    if not os.path.exists(os.path.join(args.scratch, "data", "dev")):
        shutil.copytree(os.path.join(ref_root, "data", "dev"), os.path.join(args.scratch, "data", "dev"))
    if not os.path.exists(os.path.join(args.scratch, "data", "game")):
        with zipfile.ZipFile(os.path.join(ref_root, "data", "game.zip")) as z:
            z.extractall(os.path.join(args.scratch, "data"))
    os.chdir(args.scratch)  # reference resolves ./data and ./generated from cwd
    sys.path.insert(0, ref_root)
    import torch

    torch.set_num_threads(1)
    import recad

    recad.utils.TQDM = False
    jobs = {
        "lgn_dev": lambda: golden_lightgcn(recad, torch, "dev", 64, 3, "dev_d64"),
        "lgn_dev2": lambda: golden_lightgcn(recad, torch, "dev", 128, 2, "dev_d128_l2_tg", graph_from_train=True, epochs=3),
        "lgn_game": lambda: golden_lightgcn(recad, torch, "game", 64, 3, "game_d64", row_stride=8, eval_stride=8),
        "lgn_game_tg": lambda: golden_lightgcn(recad, torch, "game", 64, 3, "game_d64_tg", row_stride=8, eval_stride=8,
                                               graph_from_train=True),
        "mf_dev": lambda: golden_mf(recad, torch, "dev", 64, "dev_e64"),
        "mf_game": lambda: golden_mf(recad, torch, "game", 64, "game_e64", max_steps=24, row_stride=8, eval_stride=8),
        "ncf_dev": lambda: golden_ncf(recad, torch, "dev", 8, 3, "dev_f8_l3"),
        "ncf_game": lambda: golden_ncf(recad, torch, "game", 32, 5, "game_f32_l5", max_steps=6, row_stride=32, eval_stride=16,
                                            dense_stride=7),
        # BASELINE.json config 5: NCF on Amazon-game at factor_num=256 (MLP tables [., 1024] / [., 4096])
        "ncf_game_f256_l3": lambda: golden_ncf(recad, torch, "game", 256, 3, "game_f256_l3", max_steps=3, row_stride=128, eval_stride=1,
                                               dense_stride=211, eval_max_users=24),
        "ncf_game_f256_l5": lambda: golden_ncf(recad, torch, "game", 256, 5, "game_f256_l5", max_steps=2, row_stride=256, eval_stride=1,
                                               dense_stride=3001, eval_max_users=3),
        # ... and the reference's evaluation of the UNTRAINED victim at the seeded initial parameters, at the reference's default
        # depth (default.py:124-125 num_layers = 5) and at 3: 64 eligible users each
        "ncf_game_f256_l5_init": lambda: golden_ncf_init_eval(recad, torch, "game", 256, 5, "game_f256_l5", 64),
        "ncf_game_f256_l3_init": lambda: golden_ncf_init_eval(recad, torch, "game", 256, 3, "game_f256_l3", 64),
        "inject_dev": lambda: golden_graph_inject(recad, torch, "dev", "dev"),
    }
    for k, fn in jobs.items():
        if args.only and k not in args.only.split(","):
            continue
        fn()


if __name__ == "__main__":
    main()
