"""GPU tests of the held-out ranking metrics: rk_rank_metrics against the float64 restatement (tests/_rank_restate.py), its
refusals, the rank_metrics / heldout_quality wrappers, EvalSession(quality=...) and the `quality_split` workflow key.

Shapes.  K = 1, 63, 64, 65 (around one 64-position chunk), 100 (the workflows') and 129 (three chunks); n = 1, 4, 5 (the
four-wave workgroup edge) and 1025 (more than one pass of the 1024-thread reduction); cut-offs {1}, {K}, {1, 64, 65, K} clipped
to K, and eight in descending order.  Crafted rows: _rank_restate.crafted.

Bounds (none is a measurement).  hits, first and out[0] are integers: equality.  dcg of a row adds at most K terms, none above
1, in double in another order than the restatement: relative K * 2^-52.  Every sum of out adds at most n such quotients:
relative (n + K) * 2^-52."""
import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, model, synth, workflow
from recad_amd.evaluate import EvalSession, eligible_users, full_catalog_topk, heldout_quality, quality_dict, rank_metrics

from . import _rank_restate as R

pytestmark = pytest.mark.gpu
EINVAL = -22
U = 2.0 ** -52
NAMES = ("Recall", "Precision", "NDCG", "HitRate", "MRR")


def _t(a, dtype, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _call(dev, top, users, ptr, idx, ks, disc, n=None, K=None, nk=None, null=()):
    """rk_rank_metrics on device copies -> (rc, hits, dcg, first, out) with sentinel-filled outputs."""
    n_, K_ = top.shape
    a = {"top": _t(top, np.int32, dev), "users": _t(users, np.int32, dev), "ptr": _t(ptr, np.int32, dev),
         "idx": _t(np.append(idx, 0), np.int32, dev), "ks": _t(ks, np.int32, dev), "disc": _t(disc, np.float64, dev),
         "hits": torch.full((max(n_, 1), len(ks)), -7, dtype=torch.int32, device=dev),
         "dcg": torch.full((max(n_, 1), len(ks)), -7.0, dtype=torch.float64, device=dev),
         "first": torch.full((max(n_, 1),), -7, dtype=torch.int32, device=dev),
         "out": torch.full((1 + 5 * len(ks),), -7.0, dtype=torch.float64, device=dev)}
    p = {k: (None if k in null else _lib.ptr(v)) for k, v in a.items()}
    rc = _lib.lib().rk_rank_metrics(p["top"], n_ if n is None else n, K_ if K is None else K, p["users"], p["ptr"], p["idx"], p["ks"],
                                    len(ks) if nk is None else nk, p["disc"], p["hits"], p["dcg"], p["first"], p["out"], _lib.stream_ptr())
    torch.cuda.synchronize()
    return (rc,) + tuple(a[k].cpu().numpy() for k in ("hits", "dcg", "first", "out"))


def _close(got, ref, rel):
    return bool(np.all(np.abs(got - ref) <= rel * np.abs(ref)))


@pytest.mark.parametrize("n", [1, 4, 5, 1025])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 100, 129])
def test_entry_point_against_the_restatement(gpu_device, K, n):
    case = R.crafted(K, n)
    disc = R.discount_table(K)
    for ks in R.cutoff_sets(K):
        rc, hits, dcg, first, out = _call(gpu_device, *case, ks, disc)
        r_hits, r_dcg, r_first, r_out = R.rank_metrics(*case, ks, disc)
        err_d = float(np.max(np.abs(dcg[:n] - r_dcg) / np.maximum(np.abs(r_dcg), 1e-300)))
        err_o = float(np.max(np.abs(out - r_out) / np.maximum(np.abs(r_out), 1e-300)))
        print(f"K={K} n={n} ks={ks}: dcg rel err {err_d:.3e} (bound {K * U:.3e}), out rel err {err_o:.3e} (bound {(n + K) * U:.3e})")
        assert rc == 0
        assert np.array_equal(hits[:n], r_hits) and np.array_equal(first[:n], r_first) and out[0] == r_out[0], (K, n, ks)
        assert _close(dcg[:n], r_dcg, K * U), (K, n, ks, err_d)
        assert _close(out, r_out, (n + K) * U), (K, n, ks, err_o)


def test_a_cutoff_outside_the_list_is_clamped(gpu_device):
    K = 65
    case = R.crafted(K, 40)
    disc = R.discount_table(K)
    rc, hits, dcg, first, out = _call(gpu_device, *case, [0, -3, 66, 1000], disc)
    ref = R.rank_metrics(*case, [1, 1, 65, 65], disc)
    assert rc == 0 and np.array_equal(hits, ref[0]) and np.array_equal(first, ref[2]) and _close(out, ref[3], (40 + K) * U)


def test_refusals_and_the_empty_call(gpu_device):
    K = 10
    case = R.crafted(K, 5)
    disc, ks = R.discount_table(K), [1, 10]
    untouched = lambda r: (r[1] == -7).all() and (r[2] == -7).all() and (r[3] == -7).all() and (r[4] == -7).all()
    for kw in ({"n": -1}, {"K": 0}, {"K": 257}, {"nk": 0}, {"nk": 9}):
        r = _call(gpu_device, *case, ks, disc, **kw)
        assert r[0] == EINVAL and untouched(r), kw
    for name in ("top", "users", "ptr", "idx", "ks", "disc", "hits", "dcg", "first", "out"):
        r = _call(gpu_device, *case, ks, disc, null=(name,))
        assert r[0] == EINVAL and untouched(r), name
    # n == 0: out is all zeros, nothing else is touched -- also with every other pointer null
    r = _call(gpu_device, *case, ks, disc, n=0)
    assert r[0] == 0 and (r[4] == 0).all() and (r[1] == -7).all() and (r[2] == -7).all() and (r[3] == -7).all()
    r = _call(gpu_device, *case, ks, disc, n=0, null=("top", "users", "ptr", "idx", "ks", "disc", "hits", "dcg", "first"))
    assert r[0] == 0 and (r[4] == 0).all()


def test_rank_metrics_wrapper(gpu_device):
    K, n = 100, 40
    top, users, ptr, idx = R.crafted(K, n)
    topks = (50, 10, 100)
    ref = quality_dict(R.rank_metrics(top, users, ptr, idx, topks, R.discount_table(K))[3], topks)
    top_d = _t(top, np.int32, gpu_device)
    host = rank_metrics(top_d, users, ptr, idx, topks)
    dev = rank_metrics(top_d, _t(users, np.int32, gpu_device), _t(ptr, np.int32, gpu_device), _t(idx, np.int32, gpu_device), topks)
    assert list(host) == [f"{m}@{k}" for k in topks for m in NAMES] + ["n_quality_users"]
    assert host == dev and host["n_quality_users"] == ref["n_quality_users"] == int(np.count_nonzero(np.diff(ptr)[users]))
    for k, v in ref.items():
        assert abs(host[k] - v) <= (n + K) * U * abs(v), k
    hits, dcg, first, out = rank_metrics(top_d, users, ptr, idx, topks, to_host=False)
    assert all(t.is_cuda for t in (hits, dcg, first, out)) and tuple(hits.shape) == (n, 3) and tuple(out.shape) == (16,)
    assert quality_dict(out.cpu().numpy(), topks) == host
    # an unsorted host row with a duplicate is canonicalised: user 3's list reversed, its first item once more
    b, e = int(ptr[3]), int(ptr[4])
    idx2 = np.concatenate([idx[:b], idx[b:e][::-1], idx[b:b + 1], idx[e:]])
    ptr2 = ptr.copy()
    ptr2[4:] += 1
    assert rank_metrics(top_d, users, ptr2, idx2, topks) == host
    for bad in ((0, 10), (10, 101), (-1,), ()):
        with pytest.raises(ValueError):
            rank_metrics(top_d, users, ptr, idx, bad)
    with pytest.raises(ValueError):
        rank_metrics(top_d, users, ptr, idx, tuple(range(1, 10)))
    # the lists are taken as int32 on the device: anything else (torch.topk's int64 indices, a host array) is refused, not misread
    for bad in (top_d.long(), top_d.cpu(), top, top_d[0]):
        with pytest.raises(TypeError):
            rank_metrics(bad, users, ptr, idx, topks)
    assert rank_metrics(top_d.t().contiguous().t(), users, ptr, idx, topks) == host   # a strided view is made contiguous


def _tiny(dev, sample, need_graph, seen_in_test=False, seed=5):
    d = synth.make("tiny")
    test = d["test"]
    if seen_in_test:   # the first train item of users 0..9 is ALSO held out: never recommended, still counted in |gt|
        tp, ti = (np.asarray(a) for a in d["train"])
        ptr, idx = (np.asarray(a) for a in test)
        rows = [np.append(idx[ptr[u]:ptr[u + 1]], ti[tp[u]] if u < 10 and tp[u + 1] > tp[u] else []).astype(np.int32) for u in range(len(ptr) - 1)]
        test = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), np.concatenate(rows))
    return dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=test, need_graph=need_graph,
                               device=dev, sample=sample, graph_source="train", seed=seed)


@pytest.mark.parametrize("name", ["lightgcn", "mf", "ncf"])
def test_heldout_quality_on_tiny(gpu_device, name):
    ds = _tiny(gpu_device, "pairwise" if name == "lightgcn" else "pointwise", name == "lightgcn", seen_in_test=True)
    kw = {"lightgcn": {"latent_dim_rec": 32}, "mf": {"embedding_size": 32}, "ncf": {"factor_num": 8, "num_layers": 2}}[name]
    torch.manual_seed(3)
    v = model.from_config("victim", name, **kw).I(dataset=ds).to(gpu_device)
    v.train_step(progress_bar=None)
    topks = (10, 20, 50, 100)
    for split in ("test", "valid"):
        got = heldout_quality(v, ds, split=split, topks=topks)
        gt_ptr, gt_idx = ds.heldout_csr(split)
        users = np.nonzero(np.diff(gt_ptr))[0].astype(np.int32)
        seen_ptr, seen_idx = ds.train_csr_sorted()
        top = full_catalog_topk(v, users, seen_ptr, seen_idx, np.zeros(0, dtype=np.int32), K=100)["top_ids"]
        ref = quality_dict(R.rank_metrics(top, users, gt_ptr, gt_idx, topks, R.discount_table(100))[3], topks)
        assert got["n_quality_users"] == len(users) == ref["n_quality_users"] > 0, (name, split)
        for k, r in ref.items():
            assert abs(got[k] - r) <= (len(users) + 100) * U * abs(r), (name, split, k)
        assert 0 < got["Recall@100"] <= 1 and got["Recall@10"] <= got["Recall@100"]
    # a held-out item of the seen list is never listed and stays in |gt|
    sp, si = ds.train_csr_sorted()
    tp, ti = ds.heldout_csr("test")
    assert all(si[sp[u]] in ti[tp[u]:tp[u + 1]] for u in range(10) if sp[u + 1] > sp[u])
    users = np.arange(10, dtype=np.int32)
    top = full_catalog_topk(v, users, sp, si, np.zeros(0, dtype=np.int32), K=100)["top_ids"]
    assert not any(si[sp[u]] in top[u] for u in range(10) if sp[u + 1] > sp[u])
    sub = heldout_quality(v, ds, topks=topks, users=np.arange(20))
    assert sub["n_quality_users"] == int(np.count_nonzero(np.diff(tp)[:20]))


def test_eval_session_quality(gpu_device):
    ds = _tiny(gpu_device, "pairwise", True)
    torch.manual_seed(3)
    v = model.from_config("victim", "lightgcn", latent_dim_rec=32).I(dataset=ds).to(gpu_device)
    v.train_step(progress_bar=None)
    ptr, idx = ds.train_csr_sorted()
    targets = np.array([0], dtype=np.int32)
    users = eligible_users(ptr, idx, targets)
    topks = (10, 20, 50, 100)
    gt = ds.heldout_csr("test")
    sess = EvalSession(v, users, ptr, idx, targets, K=100, topks=topks, quality=gt)
    outs = []
    for _ in range(3):   # eager, capture, replay
        res = sess.run()
        outs.append(res["quality_out"].cpu().numpy().copy())
    assert sess._graph is not None, "the second run must have captured the evaluation"
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    ref = R.rank_metrics(res["top_ids"].cpu().numpy(), users, *gt, topks, R.discount_table(100))[3]
    assert outs[0][0] == ref[0] > 0 and _close(outs[0], ref, (len(users) + 100) * U)
    plain = EvalSession(v, users, ptr, idx, targets, K=100, topks=topks)
    assert set(plain.run()) == {"top_ids", "top_scores", "target_score", "target_rank", "hit_counts"}
    assert set(res) == set(plain.run()) | {"quality_out"}


def _run_workflow(dev, quality_split):
    torch.manual_seed(7)
    np.random.seed(7)
    ds = _tiny(dev, "pairwise", True, seed=11)
    wf = workflow.from_config("no defense", victim_data=ds, attack_data=None,
                              victim=model.from_config("victim", "lightgcn", latent_dim_rec=32, deterministic=True),
                              attacker=workflow.RandomAttack(ds.n_items, attack_num=20, filler_num=10, seed=2),
                              rec_epoch=2, attack_epoch=0, device=dev, quality_split=quality_split)
    return wf, ds, wf.execute()


def test_workflow_quality_split(gpu_device):
    topks = [10, 20, 50, 100]
    wf, ds, res = _run_workflow(gpu_device, "test")
    clean, after = heldout_quality(wf.victim, ds, topks=topks), heldout_quality(wf.fake_victim, ds, topks=topks)
    for k in topks:
        for m in NAMES:
            assert res[f"{m}@{k}"] == clean[f"{m}@{k}"] and res[f"{m}@{k} after attack"] == after[f"{m}@{k}"], (m, k)
    assert res["n_quality_users"] == clean["n_quality_users"] == int(np.count_nonzero(np.diff(ds.heldout_csr("test")[0])))
    old = ["pred_shift"] + [f"HR@{k}{s}" for k in topks for s in ("", " after attack")] + ["n_eval_users"]
    assert list(res)[: len(old)] == old and len(res) == len(old) + 10 * len(topks) + 1
    assert all(np.isfinite(v) for v in res.values()) and res["Recall@100"] > 0
    # normal_evaluate keeps nothing between calls: other models and cut-offs get their own numbers
    direct = wf.normal_evaluate(wf.fake_victim, wf.victim, ds, [0], [5, 10])
    swapped = heldout_quality(wf.fake_victim, ds, topks=[5, 10]), heldout_quality(wf.victim, ds, topks=[5, 10])
    for k in (5, 10):
        for m in NAMES:
            assert direct[f"{m}@{k}"] == swapped[0][f"{m}@{k}"] and direct[f"{m}@{k} after attack"] == swapped[1][f"{m}@{k}"], (m, k)
    _, _, res0 = _run_workflow(gpu_device, None)
    assert list(res0) == old
    assert all(res0[k] == res[k] for k in old), {k: (res0[k], res[k]) for k in old if res0[k] != res[k]}


def test_defense_workflow_quality_split(gpu_device):
    ds = _tiny(gpu_device, "pairwise", True)
    defender = model.from_config("defender", "PCASelectUsers", attack_num=15, device=gpu_device)
    wf = workflow.from_config("defense", victim_data=ds, attack_data=None, victim=model.from_config("victim", "lightgcn", latent_dim_rec=32),
                              attacker=workflow.RandomAttack(ds.n_items, attack_num=15, filler_num=8, seed=3),
                              defender=defender, rec_epoch=2, attack_epoch=0, device=gpu_device, quality_split="valid")
    res = wf.execute()
    keys = [f"{m}@{k}{s}" for k in (10, 20, 50, 100) for m in NAMES for s in ("", " after attack")] + ["n_quality_users"]
    for part in ("attacked", "defended"):
        assert all(k in res[part] and np.isfinite(res[part][k]) for k in keys), part
    # the clean model is scored once per execute(): both stages carry the same clean numbers
    assert all(res["attacked"][k] == res["defended"][k] for k in keys if not k.endswith(" after attack"))
    clean = heldout_quality(wf.victim, ds, split="valid")
    defended = heldout_quality(wf.defended_victim, ds, split="valid")
    assert all(res["defended"][k] == clean[k] and res["defended"][k + " after attack"] == defended[k] for k in clean if k != "n_quality_users")
