"""GPU tests of the FraudarSelectUsers defender end to end: defense_step on synth `tiny` plus 40 planted users against the
restatement on Python integers (tests/_fraudar_restate.py): the flagged ids, the words of the peel and the blocks, for both
weights and both selects, from every kind of dataset the defender takes; n_blocks; the empty matrix; a device refusal; one
workflow.Defense run.  Everything is exact."""
import functools

import numpy as np
import pytest
import torch

from recad_amd import dataset, model, synth, workflow
from recad_amd.defense.pca_select_users import flag_count
from recad_amd.evaluate import detection_quality
from tests import _fraudar_restate as R

pytestmark = pytest.mark.gpu
U, I, N_FAKE = 340, 200, 40


@functools.lru_cache(maxsize=None)
def _graph():
    """(ptr, idx, items): `tiny` train plus 40 users (ids 300...) who all rate the 40 least-rated items."""
    d = synth.make("tiny")
    ptr, idx = (np.asarray(a) for a in d["train"])
    ptr, idx = ptr[:301].astype(np.int64), idx[: ptr[300]].astype(np.int64)
    items = np.sort(np.argsort(R.degrees(idx, I), kind="stable")[:N_FAKE])
    return np.concatenate([ptr, ptr[-1] + N_FAKE * np.arange(1, N_FAKE + 1)]), np.concatenate([idx] + [items] * N_FAKE).astype(np.int32), items


@functools.lru_cache(maxsize=None)
def _want(kind):
    ptr, idx, _ = _graph()
    w = R.weight_table(U, kind)[R.degrees(idx, I)]
    return w, R.peel(U, I, ptr, idx, w)


def _check(d, flagged, kind, select):
    ptr, idx, items = _graph()
    w, (order, step_of, f_trace, best) = _want(kind)
    m = flag_count(N_FAKE, U)
    assert flagged == R.flagged(U, I, ptr, idx, kind, select=select, m=m)
    assert np.array_equal(d.order.cpu().numpy(), order) and np.array_equal(d.step_of.cpu().numpy(), step_of)
    assert d.info.cpu().tolist() == list(best) + [int(f_trace[0])]
    assert np.array_equal(d.w_item.cpu().numpy().view(np.uint32), w)
    (b,) = d.blocks
    users, want_items = R.block_of(step_of, best[0], U)
    assert np.array_equal(b["users"], users) and np.array_equal(b["items"], want_items)
    assert (b["t_best"], b["f_best"], b["n_best"]) == best and b["density"] == best[1] / (best[2] * 2.0 ** 24)
    assert d.predLabels.sum() == len(flagged) and all(d.predLabels[u] == 1 for u in flagged)
    rank = d.ranking
    assert [u for u, _ in rank] == R.select_count(order, U, U) and all(step_of[u] == t for u, t in rank)
    if kind == "log":
        assert best[0] == 460 and users.tolist() == list(range(300, 340)) and np.array_equal(want_items, items)
        assert select == "count" or flagged == list(range(300, 340))


@pytest.mark.parametrize("select", ["block", "count"])
@pytest.mark.parametrize("kind", ["log", "degree"])
def test_defense_step_equals_the_restatement(gpu_device, kind, select):
    """From an ImplicitData, a CSR tuple without n_items, a dense array, and an ExplicitData whose ratings 1..5 count as edges."""
    ptr, idx, _ = _graph()
    nothing = (np.zeros(U + 1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    implicit = dataset.from_config("implicit", "fd", train_csr=(ptr, idx), valid_csr=nothing, test_csr=nothing, need_graph=False,
                                   device=gpu_device, seed=5)
    ratings = np.random.default_rng(2).integers(1, 6, size=len(idx)).astype(np.float32)
    explicit = dataset.from_config("explicit", "fd", device=gpu_device, train_csr=(ptr, idx, ratings),
                                   test_csr=(nothing[0], nothing[1], np.zeros(0, dtype=np.float32)))
    dense = np.zeros((U, I), dtype=np.float32)
    dense[np.repeat(np.arange(U), np.diff(ptr)), idx] = ratings
    assert implicit.n_users == explicit.n_users == U and implicit.n_items == explicit.n_items == I
    for ds in (implicit, (ptr, idx, np.ones(len(idx), dtype=np.float32)), dense, explicit):
        d = model.from_config("defender", "FraudarSelectUsers", weight=kind, select=select, attack_num=N_FAKE, device=gpu_device).I(dataset=ds)
        flagged = d.defense_step()
        _check(d, flagged, kind, select)
    first = (d.order.clone(), d.step_of.clone(), d.info.clone())
    assert d.defense_step() == flagged and all(torch.equal(a, b) for a, b in zip(first, (d.order, d.step_of, d.info)))
    # handed over at the step, as the defence workflow does
    d = model.from_config("defender", "FraudarSelectUsers", weight=kind, select=select, attack_num=N_FAKE, device=gpu_device).I(dataset=None)
    _check(d, d.defense_step(dataset=implicit), kind, select)


def test_two_blocks(gpu_device):
    ptr, idx, items = _graph()
    want = R.blocks(U, I, ptr, idx, n_blocks=2)
    d = model.from_config("defender", "FraudarSelectUsers", n_blocks=2, device=gpu_device).I(dataset=(ptr, idx, np.ones(len(idx), dtype=np.float32), I))
    flagged = d.defense_step()
    assert len(want) == len(d.blocks) == 2 and flagged == R.flagged(U, I, ptr, idx, n_blocks=2)
    assert flagged[:N_FAKE] == list(range(300, 340)) and len(flagged) > N_FAKE
    for got, w in zip(d.blocks, want):
        assert np.array_equal(got["users"], w["users"]) and np.array_equal(got["items"], w["items"])
        assert all(got[k] == w[k] for k in ("t_best", "f_best", "n_best", "density"))
    assert np.array_equal(d.step_of.cpu().numpy(), _want("log")[1][1]), "the attributes describe the first round"
    # a round without a block ends the rounds: one edge, four rounds asked for
    d = model.from_config("defender", "FraudarSelectUsers", n_blocks=4, device=gpu_device).I(
        dataset=(np.array([0, 1, 1]), np.array([1]), np.ones(1, dtype=np.float32), 2))
    assert d.defense_step() == [0] and len(d.blocks) == 1 and d.blocks[0]["items"].tolist() == [1]


def test_empty_matrix_and_refusals(gpu_device):
    for ds in ((np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32), 4), np.zeros((5, 4), dtype=np.float32)):
        for select in ("block", "count"):
            d = model.from_config("defender", "FraudarSelectUsers", select=select, device=gpu_device).I(dataset=ds)
            assert d.defense_step() == [] and d.blocks == [] and d.predLabels.tolist() == [0.0] * 5 and d.ranking is None
    ptr, idx, _ = _graph()
    bad = np.ones(len(idx), dtype=np.float32)
    bad[ptr[41] + 1] = 2.5
    d = model.from_config("defender", "FraudarSelectUsers", device=gpu_device).I(dataset=(ptr, idx, bad, I))
    with pytest.raises(ValueError, match=r"rule 1 .*row 41"):
        d.defense_step()
    assert d.step_of is None and d.blocks == []
    # one more item nobody rated: ln(0 + 1.5) < 1, a weight above 2^24, refused on the device at the lowest column length met
    d = model.from_config("defender", "FraudarSelectUsers", log_offset=1.5, device=gpu_device).I(
        dataset=(ptr, idx, np.ones(len(idx), dtype=np.float32), I + 1))
    with pytest.raises(ValueError, match=r"rule 19 .*index 0 .*log_offset"):
        d.defense_step()
    assert d.step_of is None and d.blocks == []
    too_many = (np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32), R.MAX_NODES)
    with pytest.raises(ValueError, match="RK_FD_MAX_NODES"):
        model.from_config("defender", "FraudarSelectUsers", device=gpu_device).I(dataset=too_many).defense_step()


class PlantedAttack(workflow.RandomAttack):
    """RandomAttack's interface; every fake profile rates the attack_num least-rated items of the clean train set 5."""

    def __init__(self, n_items, items, attack_num):
        super().__init__(n_items, attack_num=attack_num, seed=0)
        self.items = items

    def generate_fake(self, target_id_list, **config):
        fake = np.zeros((self.attack_num, self.n_items), dtype=float)
        fake[:, self.items] = 5
        return fake


def test_defense_workflow_with_fraudar_defender(gpu_device):
    d = synth.make("tiny")
    ds = dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                             device=gpu_device, need_graph=False, sample="pointwise", seed=5)
    _, _, items = _graph()
    defender = model.from_config("defender", "FraudarSelectUsers", device=gpu_device)
    wf = workflow.from_config("defense", victim_data=ds, attack_data=None, victim=model.from_config("victim", "mf"),
                              attacker=PlantedAttack(ds.n_items, items, N_FAKE), defender=defender, rec_epoch=2, attack_epoch=0,
                              device=gpu_device)
    res = wf.execute()
    assert set(res) == {"attacked", "defended", "n_flagged"} and wf.fake_dataset.n_users == U
    ptr, idx = wf.fake_dataset.train_csr_sorted()
    want = R.flagged(U, I, np.asarray(ptr)[: U + 1].astype(np.int64), np.asarray(idx)[: int(ptr[U])].astype(np.int64))
    assert res["n_flagged"] == len(want) == N_FAKE
    assert wf.detection == detection_quality(want, 300, U)
    assert wf.detection["n_fake"] == N_FAKE and wf.detection["true_positives"] == N_FAKE and wf.detection["f1"] == 1.0
