"""CPU tests of the AushPlus attacker's host side (recad_amd/attack/aushplus.py): the registry against the reference's values,
the lazy-init contract, every configuration it refuses, the loud failure without a HIP device, the template draw against a dense
restatement of build_network (aushplus.py:23-31) under the same numpy seed, the weight initialisation's draw order, the packed
layouts, and the float64 restatement the GPU tests lean on (tests/_aushplus_restate.py) against closed forms."""
import numpy as np
import pytest
import torch
from torch import nn

from recad_amd import dataset, default, model
from recad_amd.attack import aushplus as ap
from recad_amd.utils import InstantiateFail, NotInstantiatedError
from tests import _aushplus_restate as R

# recad/default.py:187-209
REFERENCE_AUSHPLUS = {"attack_num": 50, "pretrain_epoch_g": 1, "pretrain_epoch_d": 5, "epoch_gan_d": 5, "epoch_gan_g": 1,
                      "epoch_surrogate": 50, "filler_num": 36, "lr_g": 0.01, "lr_d": 0.001, "optim_g": "adam", "optim_d": "adam",
                      "surrogate_model": "WMF", "epoch_s": 50, "unroll_steps_s": 1, "hidden_dim_s": 16, "lr_s": 1e-2,
                      "weight_decay_s": 1e-5, "batch_size_s": 16, "weight_pos_s": 1.0, "weight_neg_s": 0.0, "selected_ids": [62]}


def _ratings(n_users=30, n_items=20, seed=0):
    rng = np.random.default_rng(seed)
    mat = np.where(rng.random((n_users, n_items)) < 0.35, rng.integers(1, 6, (n_users, n_items)), 0).astype(np.float32)
    mat[0] = 0
    mat[0, :3] = 4           # a user with only 3 ratings
    return mat


def _explicit(mat):
    u, i = np.nonzero(mat)
    kvr = np.stack([u, i, mat[u, i].astype(np.int64)], 1)
    return dataset.from_config("explicit", "toy", device="cpu", train_dict=kvr)


def test_registry_and_default_keys():
    cfg = default.MODEL["attacker"]["aushplus"]
    for k, v in REFERENCE_AUSHPLUS.items():
        assert cfg[k] == v, k
    assert cfg["history_bytes"] == 1 << 30
    assert set(cfg) == set(REFERENCE_AUSHPLUS) | {"history_bytes", "logging_level", "device"}
    assert isinstance(model.from_config("attacker", "aushplus"), ap.AushPlus)
    assert ap.AushPlus.scope == "attacker" and ap.AushPlus.victim_name == "aushplus"


def test_lazy_contract_and_no_device(monkeypatch):
    lazy = model.from_config("attacker", "aushplus", filler_num=4, nonsense=3)
    assert lazy._init_config["filler_num"] == 4 and "nonsense" not in lazy._init_config
    for call in (lambda: lazy.train_step(target_id_list=[0]), lambda: lazy.generate_fake(target_id_list=[0]), lazy.input_describe,
                 lazy.output_describe, lazy.pretrain_G, lazy.train_D):
        with pytest.raises(NotInstantiatedError):
            call()
    assert lazy.reset(epoch_surrogate=3)._init_config["epoch_surrogate"] == 3
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(InstantiateFail, match="HIP"):
        lazy.I(dataset=_explicit(_ratings()))


@pytest.mark.parametrize("kw, key", [
    ({"surrogate_model": "ItemAE"}, "surrogate_model"),
    ({"weight_neg_s": 0.5}, "weight_neg_s"),
    ({"optim_g": "SGD"}, "optim_g"),
    ({"hidden_dim_s": 0}, "hidden_dim_s"),
    ({"hidden_dim_s": 65}, "hidden_dim_s"),
    ({"batch_size_s": 257}, "batch_size_s"),
    ({"unroll_steps_s": 0}, "unroll_steps_s"),
    ({"unroll_steps_s": 4, "epoch_s": 3}, "unroll_steps_s"),
    ({"epoch_surrogate": -1}, "epoch_surrogate"),
    ({"attack_num": 0}, "attack_num"),
])
def test_refusals_name_the_key(kw, key):
    with pytest.raises(InstantiateFail, match=key):
        model.from_config("attacker", "aushplus", **kw).I(dataset=_explicit(_ratings()))
    with pytest.raises(InstantiateFail, match="dataset"):
        model.from_config("attacker", "aushplus").I()


@pytest.mark.parametrize("filler_num", [0, 2, 6, 50])
def test_template_draw_matches_dense_restatement(filler_num):
    mat = _ratings()
    ptr, idx, val = _explicit(mat).rating_csr()
    np.random.seed(123)
    users, kept = ap.draw_templates(ptr, idx, val, 40, filler_num)
    after = np.random.random()
    # build_network on the dense train_array, as the reference runs it
    np.random.seed(123)
    sampled = np.random.choice(range(mat.shape[0]), 40)
    templates = mat[sampled]
    for r, template in enumerate(templates):
        fillers = np.where(template)[0]
        np.random.shuffle(fillers)
        assert np.array_equal(kept[r], fillers[:filler_num])
    assert np.array_equal(users, sampled)
    assert np.random.random() == after      # the same number of draws
    lens = {len(k) for k in kept}
    assert max(lens) <= filler_num
    if filler_num == 6:
        assert 0 in users.tolist() and 3 in lens and 6 in lens      # variable length: the 3-rating user is a template


def test_weight_init_order_and_packing():
    I = 37
    torch.manual_seed(9)
    gs, ds = ap.init_weights(I)
    # the same draws, spelled out: two Linear constructions, normal_ per layer, three Linear constructions
    torch.manual_seed(9)
    l0, l1 = nn.Linear(I, 125), nn.Linear(125, I)
    w0 = torch.empty(125, I).normal_(0.0, np.sqrt(2.0 / (I + 125)))
    b0 = torch.empty(125).normal_(0.0, 0.001)
    w1 = torch.empty(I, 125).normal_(0.0, np.sqrt(2.0 / (I + 125)))
    b1 = torch.empty(I).normal_(0.0, 0.001)
    d0, d2, d4 = nn.Linear(I, 512), nn.Linear(512, 128), nn.Linear(128, 1)
    for got, want in ((gs["layers.0.weight"], w0), (gs["layers.0.bias"], b0), (gs["layers.1.weight"], w1), (gs["layers.1.bias"], b1),
                      (ds["main.0.weight"], d0.weight), (ds["main.2.bias"], d2.bias), (ds["main.4.weight"], d4.weight)):
        assert torch.equal(got, want.detach())
    assert torch.equal(gs["min_boundary_value"], torch.ones(I)) and torch.equal(gs["interval_lengths"], torch.ones(I, 3))
    assert list(gs) == ["min_boundary_value", "interval_lengths", "layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias"]
    pg, pd = ap.pack_generator(gs, I), ap.pack_discriminator(ds, I)
    assert pg.numel() == I * (2 * 128 + 5) + 128 and pd.numel() == I * 512 + 512 + 128 * 512 + 2 * 128 + 1
    assert torch.equal(pg[:I * 128].view(I, 128)[:, 125:], torch.zeros(I, 3))       # the pad columns
    for k, v in ap.unpack_generator(pg, I).items():
        assert torch.equal(v, gs[k]), k
    for k, v in ap.unpack_discriminator(pd, I).items():
        assert torch.equal(v, ds[k]), k


def test_gather_rows_and_item_lists():
    mat = _ratings()
    ptr, idx, val = _explicit(mat).rating_csr()
    ptr, idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int64)
    users = np.asarray([5, 0, 17, 5])
    rp, col, x = ap.gather_rows(ptr, idx, np.asarray(val), users)
    dense = np.zeros((4, mat.shape[1]), np.float32)
    dense[np.repeat(np.arange(4), np.diff(rp)), col] = x
    assert np.array_equal(dense, mat[users])
    rows = np.repeat(np.arange(4), np.diff(rp))
    tptr, order = ap.by_item(col, rows, mat.shape[1])
    assert np.array_equal(np.diff(tptr), (mat[users] != 0).sum(0))
    assert (np.diff(col[order]) >= 0).all()
    for j in range(mat.shape[1]):
        assert (np.diff(rows[order][tptr[j]:tptr[j + 1]]) >= 0).all()      # entry order kept inside an item


def test_restatement_projection_closed_forms():
    """At initialisation the boundaries are 1, 2.0001, 3.0002, 4.0003; the classes, the masked value and the surrogate gradient
    of the restatement against the formulas of the projection written out by hand."""
    I = 6
    gs = {"min_boundary_value": torch.ones(I), "interval_lengths": torch.ones(I, 3), "layers.0.weight": torch.zeros(125, I),
          "layers.0.bias": torch.zeros(125), "layers.1.weight": torch.zeros(I, 125),
          "layers.1.bias": torch.atanh((torch.tensor([0.5, 1.5, 2.5, 3.5, 4.5, 2.0001]) - 2.5) / 2.5)}
    g = R.params64(gs)
    b = R.boundaries(g).detach().numpy()
    eps = float(np.float32(1e-4))
    assert np.allclose(b[0], [1, 2 + eps, 3 + 2 * eps, 4 + 3 * eps], rtol=0, atol=1e-15)
    rowptr, col, x = np.asarray([0, 6]), np.arange(6), np.asarray([3, 0, 1, 5, 2, 4], np.float32)
    fw = R.g_forward(g, rowptr, col, x)
    a = fw["a"].detach().numpy()
    assert np.allclose(a[:5], [0.5, 1.5, 2.5, 3.5, 4.5], atol=1e-12)
    assert np.array_equal(fw["dist"].detach().numpy()[:5], np.eye(5))
    assert np.array_equal(fw["value"].detach().numpy()[:5], [1, 2, 3, 4, 5])
    assert np.array_equal(fw["masked"].detach().numpy()[:5], [1, 0, 3, 4, 5])          # value * [x > 0]
    # d value / d a at an interior entry of class c: sum over the active class (all four terms) and the classes with exactly
    # one failing factor (that term): entry 2 (a = 2.5, class 2)
    fw["value"][2].backward()
    d = 2.5 - b[2]
    sech2 = 1 - np.tanh(d) ** 2
    # class 2 active: +3 (s = +,+,-,-); class 1 fails only k = 1: 2 * s_11 = -; class 3 fails only k = 2: 4 * s_32 = +
    want_da = 3 * (sech2[0] + sech2[1] - sech2[2] - sech2[3]) - 2 * sech2[1] + 4 * sech2[2]
    h2 = (2.5 - 2.5) / 2.5
    got = g["layers.1.bias"].grad.numpy()[2]
    assert abs(got - want_da * 2.5 * (1 - h2 ** 2)) <= 1e-12
    assert abs(g["min_boundary_value"].grad.numpy()[2] + want_da) <= 1e-12
    # CE of 0/1 logits: log(e + 4) - [class == label - 1]
    fw = R.g_forward(R.params64(gs), rowptr, col, x)
    want = np.mean([np.log(np.e + 4) - (c == y - 1) for c, y in ((0, 3), (2, 1), (3, 5), (4, 2))] + [np.log(np.e + 4) - 0])
    # entry 5 sits within 1e-7 of boundary 1 from above or below; its class is 1 or 2, never the label 4's class 3
    assert abs(float(R.ce_loss(fw)) - want) <= 1e-12


def test_restatement_discriminator_against_torch_modules():
    I = 23
    torch.manual_seed(3)
    _, ds = ap.init_weights(I)
    net = nn.Sequential(nn.Linear(I, 512), nn.ReLU(True), nn.Linear(512, 128), nn.ReLU(True), nn.Linear(128, 1), nn.Sigmoid()).double()
    net.load_state_dict({k.replace("main.", ""): v.double() for k, v in ds.items()})
    mat = _ratings(8, I, seed=2)
    ptr = np.concatenate([[0], np.cumsum((mat != 0).sum(1))])
    r, c = np.nonzero(mat)
    p = R.d_forward(R.params64(ds, grad=False), ptr, c, mat[r, c])
    assert torch.allclose(p, net(torch.as_tensor(mat).double())[:, 0], rtol=0, atol=1e-14)
    want = nn.BCELoss()(net(torch.as_tensor(mat).double()), torch.ones(8, 1, dtype=torch.float64))
    assert abs(float(R.bce(p, 1.0)) - float(want)) <= 1e-14
