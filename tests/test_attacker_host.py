"""CPU tests of the explicit dataset and the attacker registry (recad_amd/dataset.ExplicitData, recad_amd/attack): the
reference's construction and counting rules, partial_sample against the reference's own run
(tests/golden/make_golden_aush.py), the lazy-init contract, the loud failure without a HIP device and the defender's
rating pass-through; and the fp64 restatement that the AUSH kernel tests compare against (tests/_aush_restate.py): its
gradients against torch autograd, its losses against the reference's recorded ones, and the power of its error bounds."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, model, workflow
from recad_amd.attack import aush as aush_mod
from recad_amd.defense.pca_select_users import rating_csr
from recad_amd.utils import InstantiateFail, NotInstantiatedError

from . import _aush_restate as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KVR = np.array([[0, 1, 4], [0, 3, 5], [2, 1, 2], [2, 1, 3], [1, 0, 1], [2, 6, 5]], dtype=np.int64)   # (2, 1) twice


def _explicit(**kw):
    return dataset.from_config("explicit", "toy", device="cpu", **kw)


def test_explicit_sources_agree_and_sum_duplicates(tmp_path):
    valid = np.array([[3, 2, 4]], dtype=np.int64)
    test = np.array([[1, 7, 3]], dtype=np.int64)
    a = _explicit(train_dict=KVR, valid_dict=valid, test_dict=test)
    # n_users / n_items = max id + 1 over the three splits (explicit.py:83-100)
    assert (a.n_users, a.n_items) == (4, 8)
    ptr, idx, val = a.rating_csr("train")
    assert ptr.tolist() == [0, 2, 3, 5, 5]
    assert idx.tolist() == [1, 3, 0, 1, 6] and val.tolist() == [4, 5, 1, 5, 5]   # 2 + 3 summed, like csr_matrix().toarray()
    assert a.train_size == len(KVR)
    paths = {}
    for split, arr in (("train", KVR), ("valid", valid), ("test", test)):
        p = tmp_path / f"toy_{split}.csv"
        with open(p, "w") as f:
            f.write("user_id,item_id,rating,timestamp\n")
            for u, i, r in arr:
                f.write(f"{u},{i},{r},0\n")
        paths[f"path_{split}"] = str(p)
    b = _explicit(**paths)
    c = _explicit(train_csr=(np.array([0, 2, 3, 6]), np.array([3, 1, 0, 6, 1, 1]), np.array([5, 4, 1, 5, 2, 3], dtype=np.float32)),
                  valid_csr=(np.array([0, 0, 0, 0, 1]), np.array([2]), np.array([4.0])),
                  test_csr=(np.array([0, 0, 1]), np.array([7]), np.array([3.0])))
    for d in (b, c):
        assert (d.n_users, d.n_items) == (a.n_users, a.n_items)
        for split in ("train", "valid", "test"):
            for x, y in zip(d.rating_csr(split), a.rating_csr(split)):
                assert np.array_equal(x, y), split
    assert np.array_equal(b.train_kvr, KVR)
    assert sorted(map(tuple, c.train_kvr.tolist())) == sorted({(0, 1, 4), (0, 3, 5), (1, 0, 1), (2, 1, 5), (2, 6, 5)})
    with pytest.raises(ValueError, match="no train split"):
        _explicit()


def test_train_mat_and_generate_batch_rows():
    ds = _explicit(train_dict=KVR, batch_size=2)
    mat = ds.info_describe()["train_mat"]
    assert mat.dtype == np.float32 and mat.shape == (3, 7)
    ptr, idx, val = ds.rating_csr()
    for u in range(3):
        row = np.zeros(7, dtype=np.float32)
        row[idx[ptr[u]:ptr[u + 1]]] = val[ptr[u]:ptr[u + 1]]
        assert np.array_equal(mat[u], row)
    seen = []
    for dp in ds.generate_batch(user_filter=lambda train_mat: np.where((train_mat > 0).sum(1) >= 2)[0]):
        assert dp["users"].dtype == torch.int64 and dp["users_mat"].dtype == torch.float32
        assert len(dp["users"]) <= 2
        for u, row in zip(dp["users"].tolist(), dp["users_mat"].numpy()):
            assert np.array_equal(row, mat[u])
            seen.append(u)
    assert sorted(seen) == [0, 2]
    big = dataset.from_config("explicit", "big", device="cpu", train_csr=(np.array([0, 1]), np.array([5]), np.array([3.0])),
                              test_csr=(np.array([0, 0, 0]) , np.array([], dtype=np.int32), np.array([], dtype=np.float32)),
                              dense_limit=5)
    assert big.rating_csr()[2].tolist() == [3.0]
    with pytest.raises(MemoryError, match="dense_limit"):
        big.train_mat
    assert ds.info_describe()["batch_describe"]["users_mat"][1][1] == 7


def test_partial_sample_matches_reference():
    g = np.load(os.path.join(GOLDEN, "aush_game_partial.npz"))
    ds = _explicit(train_dict=g["train_kvr"], valid_dict=g["valid_kvr"], test_dict=g["test_kvr"])
    assert (ds.n_users, ds.n_items) == (int(g["orig_n_users"]), int(g["orig_n_items"]))
    np.random.seed(int(g["seed"]))
    p = ds.partial_sample(user_ratio=float(g["user_ratio"]))
    info = p.info_describe()
    assert sorted(info["user_map"]) == g["kept_users"].tolist()
    assert [info["user_map"][int(k)] for k in g["kept_users"]] == g["kept_ids"].tolist()
    assert (p.n_users, p.n_items) == (int(g["n_users"]), int(g["n_items"]))
    assert (info["valid_interactions"], info["test_interactions"]) == (int(g["valid_interactions"]), int(g["test_interactions"]))
    for x, y in zip(p.rating_csr("train"), (g["p_ptr"], g["p_idx"], g["p_val"])):
        assert np.array_equal(x, y)
    # a reset keeps the remap
    q = p.reset(batch_size=7)
    assert q.user_map == p.user_map and q.n_users == p.n_users and q.config["batch_size"] == 7


def test_registry_defaults_and_lazy_contract(monkeypatch):
    assert isinstance(dataset.factories["explicit"], type)
    e = default.DATASET_EXPLICIT
    assert (e["batch_size"], e["sep"], e["threshold"], e["sample"], e["remap_enable"]) == (256, ",", 4, "row", False)
    cfg = default.MODEL["attacker"]["aush"]
    # recad/default.py:159-168
    ref = {"attack_num": 50, "filler_num": 36, "lr_g": 0.01, "lr_d": 0.001, "optim_g": "adam", "optim_d": "adam",
           "selected_ids": [62], "ZR_ratio": 0.2}
    assert {k: cfg[k] for k in ref} == ref and "seed" in cfg
    lazy = model.from_config("attacker", "aush", filler_num=12, not_a_key=3)
    assert lazy.model_name == "aush" and lazy._init_config["filler_num"] == 12 and "not_a_key" not in lazy._init_config
    for call in (lambda: lazy.train_step(target_id_list=[0]), lambda: lazy.generate_fake(target_id_list=[0]),
                 lambda: lazy.input_describe(), lambda: lazy.output_describe()):
        with pytest.raises(NotInstantiatedError):
            call()
    again = lazy.reset(attack_num=7)
    assert again._init_config["attack_num"] == 7 and again._init_config["filler_num"] == 12
    with pytest.raises(ValueError):
        lazy.reset(nonsense=1)
    # no HIP device: .I() fails loudly instead of falling back to the CPU
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(InstantiateFail, match="HIP"):
        lazy.I(dataset=_explicit(train_dict=KVR))


def test_random_attacker_from_registry():
    ds = _explicit(train_dict=KVR)
    att = model.from_config("attacker", "random", attack_num=4, filler_num=2).I(dataset=ds)
    assert isinstance(att, workflow.RandomAttack)
    r = KVR[:, 2].astype(np.float64)          # heuristic.py:16-17 on train_kvr
    assert att.mean == np.mean(r) and att.std == np.std(r) and att.n_items == ds.n_items
    fake = att.generate_fake(target_id_list=[1])
    assert fake.shape == (4, ds.n_items) and (fake[:, 1] == 5).all()


def test_rating_csr_passes_explicit_ratings():
    ds = _explicit(train_dict=KVR)
    U, I, rp, col, val = rating_csr(ds, torch.device("cpu"))
    ptr, idx, v = ds.rating_csr()
    assert (U, I) == (ds.n_users, ds.n_items)
    assert rp.tolist() == ptr.tolist() and col.tolist() == idx.tolist() and val.tolist() == v.tolist()
    assert not hasattr(ds, "train_csr_sorted")


def test_init_weights_follow_the_reference_order():
    torch.manual_seed(5)
    g, d = aush_mod.init_weights(9)
    torch.manual_seed(5)
    ref = [torch.nn.Linear(9, 128), torch.nn.Linear(128, 9), torch.nn.Linear(9, 150), torch.nn.Linear(150, 150),
           torch.nn.Linear(150, 150), torch.nn.Linear(150, 1)]
    assert torch.equal(g["main.0.weight"], ref[0].weight) and torch.equal(g["main.2.bias"], ref[1].bias)
    assert torch.equal(d["main.0.weight"], ref[2].weight) and torch.equal(d["main.6.weight"], ref[5].weight)
    o = aush_mod.d_offsets(9)
    assert o["end"] - o["main.0.bias"] == 150 + 150 * 150 + 150 + 150 * 150 + 150 + 150 + 1


def test_aush_desc_layout_matches_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    fields = ["n_users", "batch", "rowptr", "val", "sel", "g_w1t", "g_b2", "d_param", "d_v", "touched", "n_touched", "gslot", "work",
              "work_bytes", "lr", "eps"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "recad_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(rk_aush_desc));']
    lines += [f'printf("{f} %zu\\n", offsetof(rk_aush_desc, {f}));' for f in fields]
    lines += ['printf("limits %d %d %d %d %d\\n", RK_AUSH_HG, RK_AUSH_HD, RK_AUSH_MAX_FILLER, RK_AUSH_MAX_SELECT, RK_AUSH_MAX_PAIRS);',
              "return 0; }"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = {l.split(" ", 1)[0]: l.split(" ", 1)[1] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert C.sizeof(_lib.AushDesc) == int(out["size"])
    for f in fields:
        assert getattr(_lib.AushDesc, f).offset == int(out[f]), f
    assert out["limits"].split() == [str(x) for x in (_lib.RK_AUSH_HG, _lib.RK_AUSH_HD, _lib.RK_AUSH_MAX_FILLER,
                                                       _lib.RK_AUSH_MAX_SELECT, _lib.RK_AUSH_MAX_PAIRS)]


def test_golden_fixtures_are_consistent():
    g = np.load(os.path.join(GOLDEN, "aush_game_f12.npz"))
    assert bool(g["g_unchanged"])               # the reference never trains its generator (aush.py:138)
    assert np.array_equal(g["g_fp0"], g["g_fp_after"])
    S = g["selected_ids"].tolist()
    lens = g["batch_len"]
    p = np.load(os.path.join(GOLDEN, "aush_game_partial.npz"))
    ptr, idx, val = _explicit(train_dict=p["train_kvr"], valid_dict=p["valid_kvr"], test_dict=p["test_kvr"]).rating_csr()
    fp = [len(idx), ptr.astype(np.float64).sum(), idx.astype(np.float64).sum(), val.astype(np.float64).sum()]
    assert np.array_equal(np.asarray(fp), g["csr_fp"])           # the fixture ran on the game data stored with the partial case
    off = 0
    for b, B in enumerate(lens):
        users = g["users"][off:off + B]
        zr = g["zr"][off:off + B]
        s_real = np.array([[val[ptr[u] + np.searchsorted(idx[ptr[u]:ptr[u + 1]], s)] if s in idx[ptr[u]:ptr[u + 1]] else 0
                            for s in S] for u in users])
        n = int((s_real == 0).sum())
        assert int(zr.sum()) == n - int(np.floor(n * (1 - float(g["zr_ratio"]))))
        assert not zr[s_real != 0].any()
        off += B


# ---------------------------------------------------------------- the restatement behind tests/test_attacker_kernels_gpu.py
def _dense(c, values, I):
    """B x I rows from the sparse entries (columns [B, W] with the sentinel as padding)."""
    out = np.zeros((c.shape[0], I))
    for r in range(c.shape[0]):
        live = c[r] != R.SENTINEL
        out[r, c[r][live]] = values[r][live]
    return torch.from_numpy(out)


@pytest.mark.parametrize("B,F,S,shared", [(5, 6, 3, False), (4, 5, 3, True), (1, 7, 1, True)])
def test_restated_gradients_match_autograd(B, F, S, shared):
    """The reference's discriminator as a float64 torch module on dense B x I rows, loss 0.5 (BCE(D(real), 1) + BCE(D(fake), 0))
    with the fake rows detached: every restated gradient equals autograd's up to fp64 rounding."""
    I = 300
    P = R.craft_params(I, 11, w=1.0, b4=0.5)
    c = R.craft_rows(B, F, S, I, 12, shared=shared, sel_last=shared)
    if not shared:
        assert (c["nf"] == 0).any() and (c["nf"][1] < F)            # a row without fillers, a row with nf < F
    out = R.d_step_ref(P, I, c["fcol"], c["fval"], c["nf"], c["sval"], c["gen"], c["zr"], c["sel"])
    v = R.unpack_d(P.astype(np.float64), I)
    lins = [torch.nn.Linear(I, R.HD), torch.nn.Linear(R.HD, R.HD), torch.nn.Linear(R.HD, R.HD), torch.nn.Linear(R.HD, 1)]
    net = torch.nn.Sequential(*[m for lin in lins for m in (lin, torch.nn.Sigmoid())]).double()
    names = ["main.0", "main.2", "main.4", "main.6"]
    with torch.no_grad():
        lins[0].weight.copy_(torch.from_numpy(v["W1t"].T.copy()))
        lins[0].bias.copy_(torch.from_numpy(v["main.0.bias"]))
        for lin, n in zip(lins[1:], names[1:]):
            lin.weight.copy_(torch.from_numpy(v[n + ".weight"]))
            lin.bias.copy_(torch.from_numpy(v[n + ".bias"]))
    real, fake = _dense(out["ec"], out["ev_r"], I), _dense(out["ec"], out["ev_f"], I).detach()
    bce = torch.nn.BCELoss()
    xr, xf = net(real)[:, 0], net(fake)[:, 0]
    loss = 0.5 * (bce(xr, torch.ones(B, dtype=torch.float64)) + bce(xf, torch.zeros(B, dtype=torch.float64)))
    loss.backward()
    assert abs(float(loss.detach()) - out["losses"][0]) <= 1e-12 * out["losses"][0]
    assert abs(float(bce(xf, torch.ones(B, dtype=torch.float64))) - out["losses"][3]) <= 1e-12 * out["losses"][3]
    auto = {"main.0.weight": lins[0].weight.grad.numpy().T}
    mine = {"main.0.weight": R.unpack_d(out["g"], I)["W1t"]}
    for lin, n in zip(lins, names):
        auto[n + ".bias"] = lin.bias.grad.numpy()
        mine[n + ".bias"] = out["grad"][n + ".bias"]
        if n != "main.0":
            auto[n + ".weight"] = lin.weight.grad.numpy()
            mine[n + ".weight"] = out["grad"][n + ".weight"]
    for k in auto:
        err = np.abs(auto[k] - mine[k].reshape(auto[k].shape)).max()
        assert err <= 1e-12 * np.abs(auto[k]).max(), (k, err, np.abs(auto[k]).max())
    # the per-item table and the packed vector say the same
    assert np.array_equal(R.unpack_d(out["g"], I)["W1t"][out["items"]], out["gw1"])
    assert set(out["items"].tolist()) == set(out["ec"][out["ec"] != R.SENTINEL].tolist())


def test_restated_losses_match_the_reference_run():
    """The first batch of the reference's own run on the game data (aush_game_f12): its four losses, g_loss_gan after the
    discriminator's first Adam step, from the restatement alone."""
    g = np.load(os.path.join(GOLDEN, "aush_game_f12.npz"))
    p = np.load(os.path.join(GOLDEN, "aush_game_partial.npz"))
    ptr, idx, val = _explicit(train_dict=p["train_kvr"], valid_dict=p["valid_kvr"], test_dict=p["test_kvr"]).rating_csr()
    I, B, S = int(g["n_items"]), int(g["batch_len"][0]), np.sort(g["selected_ids"]).astype(np.int64)
    torch.manual_seed(int(g["seed"]))
    G, D = ({k: v.numpy() for k, v in st.items()} for st in aush_mod.init_weights(I))
    out = R.restate_batch_full(D, G, ptr, idx, val, g["users"][:B], g["draws"][:B], g["zr"][:B], S, I)
    grad = {k: out["grad"][k].reshape(D[k].shape) for k in R.TAIL}
    zero = {k: np.zeros(v.shape) for k, v in D.items()}
    Dn = R.adam_step64(D, zero, zero, grad, {int(c): out["gw1"][j] for j, c in enumerate(out["items"])}, 1e-3, 1, I)
    gan, _ = R.gan_loss(R.pack_d(Dn), I, *out["rows"], out["gen"], S)
    got = np.array([out["losses"][0], out["losses"][1], out["losses"][2], gan])
    assert np.all(np.abs(got - g["losses"][0]) <= 1e-5 * np.abs(g["losses"][0])), (got, g["losses"][0])


@pytest.mark.parametrize("B,shared", [(16, True), (7, False), (1, True)])
def test_error_bounds_see_the_errors_they_are_for(B, shared):
    """The bounds of the GPU comparison, applied to a deliberately damaged reference: one row's contribution missing from
    one entry (the entry where that row's contribution has the median size), a factor 2 on a whole tensor, and the fake half
    missing from one first-layer row must each fall outside; the undamaged values are inside and the bounds pass their cap."""
    I, F, S = 300, 6, 3
    P = R.craft_params(I, 21, w=R.CRAFT_W)
    c = R.craft_rows(B, F, S, I, 22, shared=shared)
    o = R.d_step_ref(P, I, c["fcol"], c["fval"], c["nf"], c["sval"], c["gen"], c["zr"], c["sel"], R.K_ULP)
    assert np.abs(o["z4"]).max() < 10
    r = 2 * B - 1                                              # the last fake row: what a loop that stops one row early drops
    contrib = {"main.6.weight": o["dz4"][r] * o["h3"][r][None, :], "main.6.bias": o["dz4"][r:r + 1], "main.4.weight": np.outer(o["dz3"][r], o["h2"][r]),
               "main.4.bias": o["dz3"][r], "main.2.weight": np.outer(o["dz2"][r], o["h1"][r]), "main.2.bias": o["dz2"][r], "main.0.bias": o["dz1"][r]}
    for k in R.TAIL:
        ref, bound = o["grad"][k], o["grad_err"][k]
        assert R.capped(ref, bound) and R.within(ref, ref, bound), k
        e = np.unravel_index(np.argsort(np.abs(contrib[k]).ravel())[contrib[k].size // 2], ref.shape)
        bad = ref.copy()
        bad[e] -= contrib[k][e]
        assert not R.within(bad, ref, bound), (k, e, contrib[k][e], bound[e])
        assert not R.within(2 * ref, ref, bound), k
    ref, bound = o["gw1"], o["gw1_err"]
    assert R.capped(ref, bound) and not R.within(2 * ref, ref, bound)
    b = B - 1                                                  # the last row's entries: the end of each of its segments
    for kk in np.nonzero(o["ec"][b] != R.SENTINEL)[0]:
        j = int(np.searchsorted(o["items"], o["ec"][b, kk]))
        whole = o["ev_r"][b, kk] * o["dz1"][b] + o["ev_f"][b, kk] * o["dz1"][B + b]
        if o["ev_f"][b, kk] == 0:
            continue                                           # a filler the user has not rated contributes an exact 0
        e = int(np.argsort(np.abs(whole))[R.HD // 2])
        for part in (whole, o["ev_f"][b, kk] * o["dz1"][B + b]):   # the row's contribution; its fake half alone
            bad = ref.copy()
            bad[j, e] -= part[e]
            assert not R.within(bad, ref, bound), (int(o["ec"][b, kk]), e)
    for i in range(4):                                         # losses: a factor 2, and one row's term missing from the mean
        assert o["loss_err"][i] <= 2.0 ** -10 * abs(o["losses"][i])
        assert not R.within(2 * o["losses"][i], o["losses"][i], o["loss_err"][i])
        assert not R.within(o["losses"][i] * (1 - 1 / (4 * B)), o["losses"][i], o["loss_err"][i])
