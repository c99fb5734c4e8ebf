"""CPU tests of the held-out ranking metrics: the float64 restatement (tests/_rank_restate.py) against a plain per-user loop
with set membership and a hand-worked case, two wrong restatements told apart, and the host side of the feature -- the
`quality_split` workflow key, the C-ABI declaration of rk_rank_metrics and the wrapper's argument checks."""
import math

import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, evaluate, synth, workflow

from . import _rank_restate as R
from .test_host_logic import _StubVictim


def loop_metrics(top_ids, user_ids, gt_ptr, gt_idx, ks, discount):
    """The definition, one user and one position at a time."""
    n, K = top_ids.shape
    nk = len(ks)
    hits, dcg, first = np.zeros((n, nk), dtype=np.int32), np.zeros((n, nk)), np.full(n, -1, dtype=np.int32)
    out = np.zeros(1 + 5 * nk)
    for b in range(n):
        u = int(user_ids[b])
        gt = set(int(i) for i in gt_idx[gt_ptr[u]:gt_ptr[u + 1]])
        if not gt:
            continue
        out[0] += 1
        for j in range(K):
            if int(top_ids[b, j]) in gt:
                if first[b] < 0:
                    first[b] = j
                for q, k in enumerate(ks):
                    if j < k:
                        hits[b, q] += 1
                        dcg[b, q] += discount[j]
        for q, k in enumerate(ks):
            idcg = sum(discount[j] for j in range(min(k, len(gt))))
            out[1 + 5 * q: 6 + 5 * q] += [hits[b, q] / len(gt), hits[b, q] / k, dcg[b, q] / idcg, float(hits[b, q] > 0),
                                          1.0 / (first[b] + 1) if 0 <= first[b] < k else 0.0]
    return hits, dcg, first, out


@pytest.mark.parametrize("K", [1, 63, 64, 65, 100, 129])
def test_restatement_equals_the_plain_loop(K):
    disc = R.discount_table(K)
    for n in (5, 40):
        case = R.crafted(K, n)
        for ks in R.cutoff_sets(K):
            got, ref = R.rank_metrics(*case, ks, disc), loop_metrics(*case, ks, disc)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and got[3][0] == ref[3][0], (K, n, ks)
            assert np.allclose(got[1], ref[1], rtol=K * 2.0 ** -52, atol=0), (K, n, ks)
            assert np.allclose(got[3], ref[3], rtol=(n + K) * 2.0 ** -52, atol=0), (K, n, ks)


def test_crafted_rows_are_what_they_claim():
    K = 100
    top, users, ptr, idx = R.crafted(K, 40)
    hits, _, first, out = R.rank_metrics(top, users, ptr, idx, [K], R.discount_table(K))
    glen = np.diff(ptr)[users]
    assert glen[0] == 0 and glen[1] == 1 and glen[2] > K and out[0] == np.count_nonzero(glen)
    assert [int(first[r]) for r in (3, 4, 5, 6)] == [0, 63, 64, K - 1] and all(hits[r, 0] == 1 for r in (3, 4, 5, 6))
    assert hits[7, 0] == K and hits[8, 0] == 0 and first[8] == -1 and (top[9] == -1).all() and first[9] == -1
    assert (top[10, K // 2:] == -1).all() and hits[10, 0] >= 1 and hits[11, 0] == 2 < glen[11]
    assert R.N_ITEMS - 1 in top[12] and hits[12, 0] == 1 and users[13] == users[3] and users[14] == users[2]


def test_hand_worked_case():
    """held-out {1, 3}, list [3, 0, 1]: hits at positions 0 and 2."""
    top = np.array([[3, 0, 1]], dtype=np.int32)
    ptr, idx = np.array([0, 2], dtype=np.int32), np.array([1, 3], dtype=np.int32)
    hits, dcg, first, out = R.rank_metrics(top, [0], ptr, idx, [1, 3], R.discount_table(3))
    res = evaluate.quality_dict(out, [1, 3])
    assert hits.tolist() == [[1, 2]] and first.tolist() == [0] and res["n_quality_users"] == 1
    assert res["Recall@1"] == 0.5 and res["HitRate@1"] == 1.0 and res["MRR@3"] == 1.0
    assert res["Precision@3"] == pytest.approx(2 / 3, rel=1e-15)
    assert res["NDCG@3"] == pytest.approx((1 + 1 / 2) / (1 + 1 / math.log2(3)), rel=1e-15)
    assert list(res) == [f"{m}@{k}" for k in (1, 3) for m in ("Recall", "Precision", "NDCG", "HitRate", "MRR")] + ["n_quality_users"]
    assert all(math.isnan(v) for k, v in evaluate.quality_dict(np.zeros(6), [5]).items() if k != "n_quality_users")


@pytest.mark.parametrize("wrong", [{"idcg_over": "k"}, {"recall_over": "min"}])
def test_a_wrong_restatement_is_rejected(wrong):
    """IDCG over k instead of min(k, |gt|) positions, and recall over min(k, |gt|): both differ from the loop on the crafted rows
    (a one-item held-out list hit at 0; a held-out list longer than K) by far more than the suites' bounds."""
    K, n = 65, 40
    disc = R.discount_table(K)
    case = R.crafted(K, n)
    ks = [1, 64, 65]
    ref = loop_metrics(*case, ks, disc)[3]
    assert np.allclose(R.rank_metrics(*case, ks, disc)[3], ref, rtol=(n + K) * 2.0 ** -52, atol=0)
    bad = R.rank_metrics(*case, ks, disc, **wrong)[3]
    assert not np.allclose(bad, ref, rtol=1e-3, atol=0)


def test_workflow_key_defaults_and_refusals():
    assert default.WORKFLOW["no defense"]["quality_split"] is None and default.WORKFLOW["defense"]["quality_split"] is None
    d = synth.make("tiny")
    ds = dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], need_graph=False,
                             device=torch.device("cpu"), seed=5)
    cfg = dict(victim_data=ds, attack_data=None, victim=_StubVictim(), attacker=workflow.RandomAttack(ds.n_items, attack_num=10, filler_num=5, seed=1),
               rec_epoch=1, attack_epoch=0, device=torch.device("cpu"))
    with pytest.raises(ValueError):
        workflow.from_config("no defense", quality_split="train", **cfg)
    res = workflow.from_config("no defense", **cfg).execute()
    assert not any(k.startswith(("Recall@", "NDCG@", "MRR@")) for k in res) and "n_quality_users" not in res
    assert list(res)[0] == "pred_shift" and list(res)[-1] == "n_eval_users"
    # a victim without a batched scoring path: no silent fall-back
    with pytest.raises(TypeError):
        workflow.from_config("no defense", quality_split="test", **cfg).execute()
    with pytest.raises(TypeError):
        evaluate.heldout_quality(_StubVictim(ds), ds)
    with pytest.raises(ValueError):
        evaluate.heldout_quality(_StubVictim(ds), ds, split="train")


def test_heldout_csr_is_sorted_and_unique():
    ds = dataset.from_config("implicit", "x", train_csr=(np.array([0, 1, 2]), np.array([0, 1], dtype=np.int32)),
                             test_csr=(np.array([0, 3, 3]), np.array([5, 2, 5], dtype=np.int32)), need_graph=False, device=torch.device("cpu"))
    ptr, idx = ds.heldout_csr("test")
    assert ptr.tolist() == [0, 2, 2] and idx.tolist() == [2, 5]
    assert ds.heldout_csr("valid")[0].tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        ds.heldout_csr("train")


def test_lib_declares_rk_rank_metrics():
    assert "rk_rank_metrics" in _lib.EXPORTS and len(_lib._SIGNATURES["rk_rank_metrics"]) == 14
    fn = _lib.lib().rk_rank_metrics
    assert fn.argtypes[1] is _lib._I64 and fn.argtypes[2] is _lib._I32 and fn.argtypes[7] is _lib._I32
    # host-side refusals need no device: nothing is launched and no pointer is followed, so a host buffer stands in for the device
    # pointers -- each refusal is then its own check's, told apart from the null-pointer one by pointers that are NOT null and
    # by the text it leaves in rk_last_error
    import ctypes as C
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)

    def refused(n, K, nk, text, ptrs=(p,) * 10):
        top, users, gptr, gidx, ks, disc, hits, dcg, first, out = ptrs
        assert fn(top, n, K, users, gptr, gidx, ks, nk, disc, hits, dcg, first, out, None) == -22, (n, K, nk)
        err = _lib.lib().rk_last_error().decode()
        assert err.startswith("rk_rank_metrics") and text in err, (n, K, nk, err)

    refused(-1, 10, 1, "n = -1")
    refused(2 ** 31, 10, 1, f"n = {2 ** 31}")
    refused(0, 0, 1, "K must be in [1,256]")
    refused(0, 257, 1, "K must be in [1,256]")
    refused(3, 10, 0, "nk must be in [1,8]")
    refused(0, 10, 9, "nk must be in [1,8]")
    for i in range(10):   # every pointer when n > 0 ...
        refused(3, 10, 2, "null pointer", (p,) * i + (None,) + (p,) * (9 - i))
    refused(0, 10, 2, "null pointer", (None,) * 10)   # ... and `out`, the one buffer still written, also when n == 0
