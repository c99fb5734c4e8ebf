"""GPU tests of the CatchSyncSelectUsers defender end to end: defense_step on a 300 x 120 graph plus 20 injected rows against
the numpy restatement (tests/_catchsync_restate.py): flagged ids, the bits of the scores, the integers and the cells, for the
three scores, both schedules and both forms, from every kind of dataset the defender takes; a refusal; one workflow.Defense run.
No detection rate is asserted here: the kernels are under test, not the statistic (tests/test_catchsync_host.py has the
detection cases)."""
import functools

import numpy as np
import pytest
import torch

from recad_amd import dataset, model, synth, workflow
from recad_amd.defense.pca_select_users import flag_count
from recad_amd.evaluate import detection_quality
from tests import _catchsync_restate as R

pytestmark = pytest.mark.gpu
U, I, N_FAKE, MIN_ITEMS, BITS = 320, 120, 20, 20, 1


@functools.lru_cache(maxsize=None)
def _graph():
    """(ptr, idx): 300 rows over 120 items whose popularity spreads over two decades (rows of 0 to about 60 items, one long
    row of 110), then 20 rows of 24 items from the 40 least popular ones.  The last item is rated and the last row is not
    empty, so that a dataset object sees the same U and I."""
    rng = np.random.default_rng(17)
    pop = np.sort(rng.random(I))[::-1]
    A = rng.random((U, I)) < 0.5 * pop[None, :]
    A[5] = False
    A[40, :110] = True
    A[300:] = False
    for f in range(N_FAKE):
        A[300 + f, 80 + rng.permutation(40)[:24]] = True
    ptr = np.concatenate([[0], np.cumsum(A.sum(axis=1))]).astype(np.int64)
    assert A[:, I - 1].any() and (np.diff(ptr)[:300] >= MIN_ITEMS).sum() > 100
    return ptr, np.nonzero(A)[1].astype(np.int32)


@functools.lru_cache(maxsize=None)
def _want(score):
    ptr, idx = _graph()
    return R.run(ptr, idx, I, score, BITS, MIN_ITEMS)


def _check(d, flagged, score):
    want = _want(score)
    m = flag_count(N_FAKE, U)
    assert flagged == R.select(want["scores"], m) and len(flagged) == m
    assert np.array_equal(d.scores.cpu().numpy().view(np.uint32), want["scores"].view(np.uint32))
    assert np.array_equal(d.pair_num.cpu().numpy(), want["pair_num"]) and np.array_equal(d.back_num.cpu().numpy(), want["back_num"])
    assert np.array_equal(d.cell_of.cpu().numpy(), want["cell_of"]) and np.array_equal(d.cell_count.cpu().numpy(), want["cell_count"])
    assert d.n_cells == want["info"][0] > 4
    assert d.predLabels.sum() == m and all(d.predLabels[u] == 1 for u in flagged)


@pytest.mark.parametrize("form", [None, "wave", "workgroup"])
@pytest.mark.parametrize("schedule", ["work", "natural"])
@pytest.mark.parametrize("score", ["sync", "normality", "residual"])
def test_defense_step_equals_the_restatement(gpu_device, score, schedule, form):
    ptr, idx = _graph()
    d = model.from_config("defender", "CatchSyncSelectUsers", score=score, grid_bits=BITS, min_items=MIN_ITEMS, attack_num=N_FAKE,
                          schedule=schedule, form=form, device=gpu_device).I(dataset=(ptr, idx, np.ones(len(idx), dtype=np.float32), I))
    flagged = d.defense_step()
    _check(d, flagged, score)
    rank = d.ranking
    want = _want(score)["scores"]
    assert [u for u, _ in rank] == R.select(want, U) and rank[0][1] == float(want[rank[0][0]])
    first = d.scores.clone()
    assert d.defense_step() == flagged and torch.equal(first, d.scores), "two calls give the same bits"


def test_every_kind_of_dataset_gives_the_same_result(gpu_device):
    """An ImplicitData, a CSR tuple without n_items, a dense array, and an ExplicitData whose ratings 1..5 count as edges."""
    ptr, idx = _graph()
    nothing = (np.zeros(U + 1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    implicit = dataset.from_config("implicit", "cs", train_csr=(ptr, idx), valid_csr=nothing, test_csr=nothing, need_graph=False,
                                   device=gpu_device, seed=5)
    ratings = np.random.default_rng(2).integers(1, 6, size=len(idx)).astype(np.float32)
    explicit = dataset.from_config("explicit", "cs", device=gpu_device, train_csr=(ptr, idx, ratings),
                                   test_csr=(nothing[0], nothing[1], np.zeros(0, dtype=np.float32)))
    dense = np.zeros((U, I), dtype=np.float32)
    dense[np.repeat(np.arange(U), np.diff(ptr)), idx] = ratings
    assert implicit.n_users == explicit.n_users == U and implicit.n_items == explicit.n_items == I
    for ds in (implicit, (ptr, idx, np.ones(len(idx), dtype=np.float32)), dense, explicit):
        d = model.from_config("defender", "CatchSyncSelectUsers", attack_num=N_FAKE, device=gpu_device).I(dataset=ds)
        assert d._init_config["grid_bits"] == BITS and d._init_config["min_items"] == MIN_ITEMS
        _check(d, d.defense_step(), "sync")
    # handed over at the step, as the defence workflow does
    d = model.from_config("defender", "CatchSyncSelectUsers", attack_num=N_FAKE, score="residual", device=gpu_device).I(dataset=None)
    _check(d, d.defense_step(dataset=implicit), "residual")


def test_kernel_refusal_names_rule_and_row(gpu_device):
    ptr, idx = _graph()
    bad = np.ones(len(idx), dtype=np.float32)
    bad[ptr[41] + 1] = 2.5
    d = model.from_config("defender", "CatchSyncSelectUsers", device=gpu_device).I(dataset=(ptr, idx, bad, I))
    with pytest.raises(ValueError, match=r"rule 1 .*row 41"):
        d.defense_step()
    assert d.scores is None and d.n_cells is None
    swapped = idx.copy()
    swapped[[ptr[7], ptr[7] + 1]] = swapped[[ptr[7] + 1, ptr[7]]]
    d = model.from_config("defender", "CatchSyncSelectUsers", device=gpu_device).I(
        dataset=(torch.from_numpy(ptr), torch.from_numpy(swapped), torch.ones(len(idx)), I))
    with pytest.raises(ValueError, match=r"rule 2 .*row 7"):
        d.defense_step()


def test_defense_workflow_with_catchsync_defender(gpu_device):
    d = synth.make("tiny")
    ds = dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                             device=gpu_device, need_graph=False, sample="pointwise", seed=5)
    defender = model.from_config("defender", "CatchSyncSelectUsers", attack_num=15, min_items=4, device=gpu_device)
    wf = workflow.from_config("defense", victim_data=ds, attack_data=None, victim=model.from_config("victim", "mf"),
                              attacker=workflow.RandomAttack(ds.n_items, attack_num=15, filler_num=40, seed=3),
                              defender=defender, rec_epoch=2, attack_epoch=0, device=gpu_device)
    res = wf.execute()
    m = flag_count(15, 315)
    assert set(res) == {"attacked", "defended", "n_flagged"}
    assert wf.fake_dataset.n_users == 315 and res["n_flagged"] == m
    ptr, idx = wf.fake_dataset.train_csr_sorted()
    want = R.run(np.asarray(ptr)[:316], np.asarray(idx)[: int(ptr[315])], ds.n_items, "sync", 1, 4)
    assert wf.detection == detection_quality(R.select(want["scores"], m), 300, 315)
    assert wf.detection["n_fake"] == 15 and wf.detection["n_flagged"] == m
