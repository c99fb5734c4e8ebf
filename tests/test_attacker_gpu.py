"""GPU tests of the AUSH attacker (csrc/aush.hip + recad_amd/attack): replay of the reference's own draws on the game
data (tests/golden/make_golden_aush.py), the device sampler's invariants, determinism, the yelp / c4s shapes against an
fp64 numpy restatement, and the attack / defence workflows.
The kernels one entry point at a time, gradients included, are in tests/test_attacker_kernels_gpu.py.

Tolerances.  The device sums in a different order than torch's CPU GEMMs and reductions (sparse first layer, per-thread
dot products, fp64 loss sums), so values agree to fp32 reordering, not to the bit: losses within 1e-5 relative (each
loss is a mean of O(B) terms of size ~1, reordering error ~1e-7); D after two epochs (10 Adam steps of lr 1e-3) within
1e-4 absolute -- an Adam step moves a weight by at most ~lr, and a reordering can only change m / sqrt(v) noticeably
where the gradient is ~1e-7 of its typical size."""
import os

import numpy as np
import pytest
import torch

from recad_amd import dataset, model, synth, workflow
from recad_amd.defense.pca_select_users import flag_count

from ._aush_restate import _restate_batch, adam_step64

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOSS_RTOL = 1e-5
D_ATOL = 1e-4


def _game(g, dev, **kw):
    """The game data as the reference loads it (its train / valid / test rows are stored with the partial_sample case);
    its train rating CSR is the one the fixture `g` recorded (in full, or as a fingerprint)."""
    p = np.load(os.path.join(GOLDEN, "aush_game_partial.npz"))
    ds = dataset.from_config("explicit", "game", train_dict=p["train_kvr"], valid_dict=p["valid_kvr"], test_dict=p["test_kvr"],
                             device=dev, **kw)
    ptr, idx, val = ds.rating_csr()
    if "csr_fp" in g:
        fp = [len(idx), ptr.astype(np.float64).sum(), idx.astype(np.float64).sum(), val.astype(np.float64).sum()]
        assert np.array_equal(np.asarray(fp), g["csr_fp"])
    else:
        for x, y in zip((ptr, idx, val), (g["ptr"], g["idx"], g["val"])):
            assert np.array_equal(x, y)
    return ds


def _rowfp(a):
    """(sum, L2 norm) per row, float64: |sum diff| <= n * atol and |norm diff| <= sqrt(n) * atol when every entry is
    within atol."""
    a = np.asarray(a, dtype=np.float64)
    return np.stack([a.sum(axis=1), np.sqrt((a * a).sum(axis=1))], axis=1)


def _fp_close(got, ref, n):
    return np.all(np.abs(got[:, 0] - ref[:, 0]) <= n * D_ATOL) and np.all(np.abs(got[:, 1] - ref[:, 1]) <= np.sqrt(n) * D_ATOL)


def _aush(ds, dev, torch_seed=2023, **kw):
    torch.manual_seed(torch_seed)
    return model.from_config("attacker", "aush", device=dev, **kw).I(dataset=ds)


def _fp(state):
    keys = sorted(state)
    return np.asarray([[state[k].double().numpy().sum(), (state[k].double().numpy() ** 2).sum()] for k in keys])


def _close(a, b, rtol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= rtol * np.abs(b))


@pytest.mark.parametrize("case", ["game_f12", "game_s3t2"])
def test_replay_of_reference_draws(gpu_device, case):
    g = np.load(os.path.join(GOLDEN, f"aush_{case}.npz"))
    ds = _game(g, gpu_device)
    assert (ds.n_users, ds.n_items) == (int(g["n_users"]), int(g["n_items"]))
    att = _aush(ds, gpu_device, torch_seed=int(g["seed"]), filler_num=int(g["filler_num"]), selected_ids=g["selected_ids"].tolist(), seed=1)
    G0 = att.generator_state()
    D0 = att.discriminator_state()
    # the initial weights are the reference's, bit for bit (same torch seed, same construction order)
    assert np.array_equal(_fp(G0), g["g_fp0"]) and np.array_equal(_fp(D0), g["d_fp0"])
    targets = g["targets"].tolist()
    assert np.array_equal(np.sort(att.eligible_users(targets)), np.unique(g["users"]))
    off, means, lens = 0, [], g["batch_len"]
    for ep in range(int(g["epochs"])):
        ep_losses = []
        for b in np.nonzero(g["batch_epoch"] == ep)[0]:
            B = int(lens[b])
            got = att.replay_batch(g["users"][off:off + B], g["draws"][off:off + B], g["zr"][off:off + B], targets)
            ref = g["losses"][b]
            assert _close(got, ref, LOSS_RTOL), (case, ep, b, got, ref.tolist())
            ep_losses.append(got)
            off += B
        means.append(np.mean(np.asarray(ep_losses, dtype=np.float64), axis=0))
        D = att.discriminator_state()
        w1, w10 = D["main.0.weight"].numpy(), D0["main.0.weight"].numpy()
        items = g[f"d{ep}_w1_items"]
        untouched = np.setdiff1d(np.arange(ds.n_items), items)
        assert np.array_equal(w1[:, untouched], w10[:, untouched])          # rows never touched: bit-equal to the init
        assert _fp_close(_rowfp(w1[:, items].T), g[f"d{ep}_w1_colfp"], 150), (case, ep, "first-layer columns")
        if f"d{ep}_w1_full_items" in g:                                    # a sample of changed columns, entry by entry
            assert np.abs(w1[:, g[f"d{ep}_w1_full_items"]].T - g[f"d{ep}_w1_full_cols"]).max() <= D_ATOL
        for k in ("main.0.bias", "main.2.weight", "main.2.bias", "main.4.weight", "main.4.bias", "main.6.weight", "main.6.bias"):
            if f"d{ep}_{k}" in g:
                assert np.abs(D[k].numpy() - g[f"d{ep}_{k}"]).max() <= D_ATOL, (case, ep, k)
            else:
                assert _fp_close(_rowfp(D[k].numpy()), g[f"d{ep}_{k}_rowfp"], D[k].shape[1]), (case, ep, k)
    assert _close(np.stack(means), g["epoch_means"], LOSS_RTOL)
    G = att.generator_state()
    assert all(torch.equal(G[k], G0[k]) for k in G0)                     # the generator never trains (aush.py:138)


def test_generate_fake_replay(gpu_device):
    g = np.load(os.path.join(GOLDEN, "aush_game_fake36.npz"))
    ds = _game(g, gpu_device)
    att = _aush(ds, gpu_device, torch_seed=int(g["seed"]), seed=1)
    targets = g["targets"].tolist()
    fake = att.replay_fake(g["users"], g["draws"], targets)
    ref = np.zeros(tuple(g["fake_shape"]), dtype=np.float32)
    ref[g["fake_rows"], g["fake_cols"]] = g["fake_vals"]
    assert fake.dtype == np.float32 and fake.shape == ref.shape
    S = g["selected_ids"].tolist()
    pre_ref = g["gen"].astype(np.float64) + np.isin(S, targets)[None, :] * 5.0
    assert np.allclose(att.last_fake["pre"], pre_ref, rtol=1e-5, atol=1e-6)
    other = np.ones(ds.n_items, dtype=bool)
    other[S] = False
    assert np.array_equal(fake[:, other], ref[:, other])                 # fillers and targets exact
    far = np.abs(pre_ref - np.floor(pre_ref) - 0.5) > 1e-4
    assert np.array_equal(fake[:, S][far], ref[:, S][far])


def _restate_eligible(ptr, idx, val, excl, F):
    out = []
    for u in range(len(ptr) - 1):
        c, v = idx[ptr[u]:ptr[u + 1]], val[ptr[u]:ptr[u + 1]]
        if int(((v > 0) & ~np.isin(c, excl)).sum()) >= F:
            out.append(u)
    return np.asarray(out)


def test_own_sampler_invariants(gpu_device):
    g = np.load(os.path.join(GOLDEN, "aush_game_f12.npz"))
    ds = _game(g, gpu_device)
    S, T, F = [7, 62, 300], [0, 5], 12
    att = _aush(ds, gpu_device, filler_num=F, selected_ids=S, seed=9)
    res = att.train_step(target_id_list=T)
    assert len(res) == len(att.output_describe()["train_step"]) and all(np.isfinite(res))
    ptr, idx, val = ds.rating_csr()
    el = _restate_eligible(ptr, idx, val, S + T, F)
    assert np.array_equal(att.eligible_users(T), el)
    pool = att._pools[tuple(sorted(T))]
    N = pool["n"]
    perm = pool["perm"].cpu().numpy()
    assert np.array_equal(np.sort(perm), el)
    r = {k: v.cpu().numpy() for k, v in pool["rows"].items()}
    fcol, nf, zr, sval = r["fcol"].reshape(N, F), r["nf"], r["zr"].reshape(N, 3), r["sval"].reshape(N, 3)
    for row, u in enumerate(perm):
        c = fcol[row, :nf[row]]
        rated = idx[ptr[u]:ptr[u + 1]][val[ptr[u]:ptr[u + 1]] > 0]
        assert 0 < nf[row] <= F and len(np.unique(c)) == nf[row]
        assert np.isin(c, rated).all() and not np.isin(c, S + T).any()
        for k, s in enumerate(S):
            pos = np.searchsorted(idx[ptr[u]:ptr[u + 1]], s)
            real = val[ptr[u] + pos] if pos < ptr[u + 1] - ptr[u] and idx[ptr[u] + pos] == s else 0.0
            assert sval[row, k] == real
    B = att.batch_size
    for b0 in range(0, N, B):
        z, sv = zr[b0:b0 + B], sval[b0:b0 + B]
        n = int((sv == 0).sum())
        assert int(z.sum()) == n - int(np.floor(n * (1 - 0.2)))
        assert not z[sv != 0].any()
    # loose uniformity: one user drawn 4000 times -- every pool item lands in the distinct set about equally often
    u = int(el[np.argmax([ptr[x + 1] - ptr[x] for x in el])])
    users = torch.full((4000,), u, dtype=torch.int32, device=gpu_device)
    rows = att._rows(4000)
    att._sample(users, rows, pool=pool, stream_id=77)
    c = rows["fcol"].cpu().numpy().reshape(4000, F)
    n = rows["nf"].cpu().numpy()
    hits = np.bincount(np.concatenate([c[i, :n[i]] for i in range(4000)]), minlength=ds.n_items)
    cand = idx[ptr[u]:ptr[u + 1]][(val[ptr[u]:ptr[u + 1]] > 0) & ~np.isin(idx[ptr[u]:ptr[u + 1]], S + T)]
    deg = len(cand)
    expect = 4000 * (1 - (1 - 1 / deg) ** F)
    h = hits[cand]
    assert hits.sum() == h.sum() and np.all(np.abs(h - expect) < 6 * np.sqrt(expect) + 5), (deg, expect, h.min(), h.max())


def test_determinism(gpu_device):
    g = np.load(os.path.join(GOLDEN, "aush_game_f12.npz"))
    ds = _game(g, gpu_device)
    out = []
    for seed in (4, 4, 5):
        att = _aush(ds, gpu_device, filler_num=12, seed=seed)
        l1 = att.train_step(target_id_list=[0])
        l2 = att.train_step(target_id_list=[0])
        fake = att.generate_fake(target_id_list=[0])
        out.append((np.concatenate([att.last_batch_losses.ravel(), l1, l2]), att.d_param.cpu().numpy(), fake))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert not np.array_equal(out[0][0], out[2][0]) and not np.array_equal(out[0][2], out[2][2])
    fake = out[0][2]
    assert fake.shape == (50, ds.n_items) and (fake[:, 0] == 5).all()
    assert set(np.unique(fake[:, 62]).tolist()) <= {1.0, 2.0, 3.0, 4.0, 5.0}


# ---------------------------------------------------------------- against the fp64 restatement (tests/_aush_restate.py)
def test_large_shapes_against_fp64(gpu_device):
    for name in ("yelp", "c4s"):
        d = synth.make_device(name, gpu_device)
        d = synth.with_ratings({k: (tuple(t.cpu().numpy() for t in v) if isinstance(v, tuple) else v) for k, v in d.items()})
        full = dataset.from_config("explicit", name, train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], device=gpu_device)
        np.random.seed(3)
        ds = full.partial_sample(user_ratio=0.2)
        att = _aush(ds, gpu_device, seed=2)
        res = att.train_step(target_id_list=[0])
        assert all(np.isfinite(res)), (name, res)
        assert np.isfinite(att.last_batch_losses).all()
        ptr, idx, val = ds.rating_csr()
        el = att.eligible_users([0])
        rng = np.random.default_rng(0)
        S, I, F = att._sel_host.tolist(), ds.n_items, att.filler_num
        G = {k: v.numpy() for k, v in att.generator_state().items()}
        for step in range(2):
            users = rng.choice(el, size=att.batch_size, replace=True)
            draws = np.stack([rng.choice(idx[ptr[u]:ptr[u + 1]][~np.isin(idx[ptr[u]:ptr[u + 1]], S + [0])], F) for u in users])
            zr = rng.integers(0, 2, size=(len(users), len(S))).astype(np.uint8)
            for r, u in enumerate(users):
                for k, s in enumerate(S):
                    if s in idx[ptr[u]:ptr[u + 1]]:
                        zr[r, k] = 0
            D = {k: v.numpy() for k, v in att.discriminator_state().items()}
            m0 = {k: v.numpy().astype(np.float64) for k, v in _moments(att, "d_m").items()}
            v0 = {k: v.numpy().astype(np.float64) for k, v in _moments(att, "d_v").items()}
            t = att._adam_t + 1
            d_loss, gen, grad, gw1, fake_fwd = _restate_batch(D, G, ptr, idx, val, users, draws, zr, S, I, att.lr_d, t)
            got = att.replay_batch(users, draws, zr, [0])
            B = len(users)
            rec = ((gen + 5) ** 2 * zr).sum() / (B * I)
            shill = (gen ** 2).sum() / (B * I)
            assert abs(got[0] - d_loss) <= 1e-5 * abs(d_loss), (name, step, got, d_loss)
            assert abs(got[1] - rec) <= 1e-5 * abs(rec) + 1e-12 and abs(got[2] - shill) <= 1e-5 * abs(shill)
            # Adam (torch.optim.Adam defaults) in fp64 on the restated gradient, then g_loss_gan with the updated D
            Dn = adam_step64(D, m0, v0, grad, gw1, att.lr_d, t, I)
            xg = fake_fwd(Dn)
            gan = -np.maximum(np.log(xg), -100).mean()
            assert abs(got[3] - gan) <= 1e-5 * abs(gan), (name, step, got[3], gan)
            Dg = att.discriminator_state()
            for k in Dn:
                assert np.abs(Dg[k].numpy() - Dn[k]).max() <= D_ATOL, (name, step, k)
        del att, ds, full, d
        torch.cuda.empty_cache()


def _moments(att, which):
    """Adam moments of D in the reference's layout (exp_avg / exp_avg_sq of netD's parameters)."""
    saved = att.d_param
    att.d_param = getattr(att, which)
    try:
        return att.discriminator_state()
    finally:
        att.d_param = saved


# ---------------------------------------------------------------- workflows
def _ml1m_data(dev):
    d = synth.make("ml1m")
    victim = dataset.from_config("implicit", "ml1m", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], device=dev,
                                 graph_source="train", seed=5)
    r = synth.with_ratings(d)
    explicit = dataset.from_config("explicit", "ml1m", train_csr=r["train"], valid_csr=r["valid"], test_csr=r["test"], device=dev)
    np.random.seed(7)
    return victim, explicit, explicit.partial_sample(user_ratio=0.2)


def test_no_defense_workflow_with_aush(gpu_device):
    victim_data, _, attack_data = _ml1m_data(gpu_device)
    wf = workflow.from_config("no defense", victim_data=victim_data, attack_data=attack_data,
                              victim=model.from_config("victim", "lightgcn", latent_dim_rec=32, lightGCN_n_layers=2),
                              attacker=model.from_config("attacker", "aush", device=gpu_device, seed=3),
                              rec_epoch=1, attack_epoch=2, target_id_list=[0], device=gpu_device)
    res = wf.execute()
    assert res["n_eval_users"] > 0
    assert all(np.isfinite(v) for v in res.values())
    assert wf.fake_dataset.n_users > victim_data.n_users


def test_defense_workflow_with_explicit_defense_data(gpu_device):
    victim_data, explicit, attack_data = _ml1m_data(gpu_device)
    wf = workflow.from_config("defense", victim_data=victim_data, attack_data=attack_data, defense_data=explicit,
                              victim=model.from_config("victim", "lightgcn", latent_dim_rec=32, lightGCN_n_layers=2),
                              attacker=model.from_config("attacker", "aush", device=gpu_device, seed=3),
                              defender=model.from_config("defender", "PCASelectUsers", device=gpu_device),
                              rec_epoch=1, attack_epoch=1, target_id_list=[0], device=gpu_device)
    res = wf.execute()
    assert wf.defender.user_num == wf.fake_dataset.n_users
    assert res["n_flagged"] == flag_count(50, wf.fake_dataset.n_users) == 50
