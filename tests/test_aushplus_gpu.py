"""GPU tests of the AushPlus attacker (csrc/aushplus.hip + recad_amd/attack/aushplus.py): every kernel against the float64
restatement of tests/_aushplus_restate.py from the device's own parameters and rows, the surrogate phase's chain, one Adam step of
each optimiser, run-to-run bit-identity, the corner shapes and both workflows.

Tolerances (derived, not measured).
  a.  a = 2.5 tanh(z) + 2.5 with z = W2_j . h1 + b2_j.  The dot products have length L1 = the row's entries (at most 2 048 in
      the shapes used here) and L2 = 125; with round-to-nearest the error of a length-L fp32 sum grows as sqrt(L) eps times the
      size of its partial sums.  The tests assert |a - 2.5| <= 1 on the restatement's side, i.e. |z| <= 0.43 (the small case has
      90 items, so its Xavier weights are five times the game data's), and the per-term products are far below that, so the
      sums carry at most sqrt(2 173) * 6e-8 * 0.43 * 2.5 = 3e-6 into a; tanhf (2 ulp at |h| < 0.5: 6e-8 * 2.5) and the two
      roundings of 2.5 h + 2.5 (2 * 2.4e-7 for a in [2, 4)) add 6e-7.  A factor 3 for the part of the error that does not
      average out gives A_TOL = 1e-5.
  class / value are compared exactly except where the restatement's min_k |a - b_k| is below MARGIN = 10 * A_TOL; such entries
      may be at most 1 % of a test's entries (asserted), and gradient comparisons drop the same entries.
  losses: means of O(100 .. 10 000) terms of size O(1), each term's error a few eps: 1e-5 relative.
  gradients: sums of up to a few thousand products with the rounding of h1 / a / D's activations in them; relative error in norm
      1e-4 per parameter tensor (sqrt(4 096) * 6e-8 = 4e-6 per sum, the chain through three layers and the 1 / norm stay well
      below 25 times that); the sign must agree where |g| is above 1e-3 of the tensor's maximum (Adam's first steps act on the
      sign).
  Adam's first step: see _check_adam (the step's conditioning in the gradient is written out there)."""
import os

import numpy as np
import pytest
import torch

from recad_amd import dataset, model, synth, workflow
from recad_amd.defense.pca_select_users import flag_count
from recad_amd.attack.aushplus import gather_rows
from tests import _aushplus_restate as R

pytestmark = pytest.mark.gpu
A_TOL = 1e-5
MARGIN = 10 * A_TOL
LOSS_RTOL = 1e-5
GRAD_RTOL = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _synth(dev, n_users=150, n_items=90, seed=3):
    rng = np.random.default_rng(seed)
    mat = np.where(rng.random((n_users, n_items)) < 0.2, rng.integers(1, 6, (n_users, n_items)), 0).astype(np.float32)
    mat[:, 0] = np.where(rng.random(n_users) < 0.3, 5, 0)         # target 0: rated by some users only
    mat[3] = 0
    mat[3, 7] = 4                                                  # a user with one rating
    mat[4] = 0
    mat[4, 1:4] = 2                                                # and one with three
    u, i = np.nonzero(mat)
    kvr = np.stack([u, i, mat[u, i].astype(np.int64)], 1)
    return dataset.from_config("explicit", "synth", device=dev, train_dict=kvr, batch_size=64), mat


def _game(dev):
    g = np.load(os.path.join(GOLDEN, "aush_game_partial.npz"))
    full = dataset.from_config("explicit", "game", device=dev, train_dict=g["train_kvr"], valid_dict=g["valid_kvr"],
                               test_dict=g["test_kvr"])
    np.random.seed(int(g["seed"]))
    return full.partial_sample(user_ratio=float(g["user_ratio"]))


def _shaped(shape, dev):
    r = synth.with_ratings(synth.make(shape))
    ds = dataset.from_config("explicit", shape, train_csr=r["train"], valid_csr=r["valid"], test_csr=r["test"], device=dev)
    np.random.seed(7)
    return ds.partial_sample(user_ratio=0.2)


def _att(ds, dev, np_seed=5, torch_seed=11, **kw):
    cfg = dict(attack_num=10, filler_num=6, epoch_s=3, unroll_steps_s=1, batch_size_s=16, pretrain_epoch_g=1, epoch_gan_d=1,
               epoch_gan_g=1, epoch_surrogate=2, device=dev)
    cfg.update(kw)
    np.random.seed(np_seed)
    torch.manual_seed(torch_seed)
    return model.from_config("attacker", "aushplus", **cfg).I(dataset=ds)


def _perturb(att, seed=0):
    """Move the boundaries and biases off their symmetric initial values so that every class and every gradient path is live."""
    g = torch.Generator().manual_seed(seed)
    gs = att.generator_state()
    I = att.n_items
    gs["min_boundary_value"] = 2.2 + 0.2 * torch.rand(I, generator=g)
    gs["interval_lengths"] = 0.12 * torch.rand(I, 3, generator=g) - 0.01          # some lengths negative: relu' = 0
    gs["layers.1.bias"] = 0.03 * torch.randn(I, generator=g)
    att.load_generator_state(gs)


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _check_grads(dev_grads, ref_grads, what):
    for k, ref in ref_grads.items():
        got, ref = np.asarray(dev_grads[k], np.float64), ref.detach().numpy()
        scale = np.abs(ref).max()
        if scale == 0:
            assert np.abs(got).max() == 0, (what, k)
            continue
        err = _relerr(got, ref)
        print(f"{what} {k}: rel err {err:.2e}, max |g| {scale:.3e}")
        assert err <= GRAD_RTOL, (what, k, err)
        big = np.abs(ref) > 1e-3 * scale
        assert np.array_equal(np.sign(got[big]), np.sign(ref[big])), (what, k)


def _check_adam(after, before, g, lr, what):
    """Adam's first step is p - lr g / (|g| + 1e-8): its sensitivity to an absolute gradient error d is lr 1e-8 d / (|g| + 1e-8)^2,
    so a small |g| is ill-conditioned.  With d = 1e-6 max|g| (well inside GRAD_RTOL in norm) plus 1e-6 for the fp32 step itself."""
    want = R.adam_first_step(before, g, lr)
    tol = 1e-6 + lr * 1e-8 * (1e-6 * np.abs(g).max()) / (np.abs(g) + 1e-8) ** 2
    assert (np.abs(after - want) <= tol).all(), what
    big = np.abs(g) > 1e-3 * np.abs(g).max()
    assert np.array_equal(np.sign(before[big] - after[big]), np.sign(g[big])), what


def _compare_forward(fw, a, cls, value, x, what):
    ra, margin = fw["a"].detach().numpy(), fw["margin"].numpy()
    assert np.abs(ra - 2.5).max() <= 1.0, "the tolerance's precondition on |z|"
    print(f"{what}: {len(ra)} entries, max |a_dev - a_ref| {np.abs(a - ra).max():.2e}, min margin {margin.min():.2e}")
    assert np.abs(a - ra).max() <= A_TOL
    keep = margin >= MARGIN
    assert (~keep).mean() <= 0.01, (what, (~keep).mean())
    dist = fw["dist"].detach().numpy()
    rcls = np.where(dist.sum(1) > 0, dist.argmax(1), -1)
    assert np.array_equal(cls[keep], rcls[keep])
    assert np.array_equal(value[keep], fw["masked"].detach().numpy()[keep].astype(np.float32))
    assert set(np.unique(value)) <= {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    return keep


def _datasets(name, dev):
    if name == "synth":
        return _synth(dev)[0]
    if name == "game":
        return _game(dev)
    return _shaped(name, dev)


# ---------------------------------------------------------------- G forward / backward
@pytest.mark.parametrize("name", ["synth", "game", "ml1m", "yelp"])
def test_generator_forward_templates_and_real_batch(gpu_device, name):
    ds = _datasets(name, gpu_device)
    att = _att(ds, gpu_device, attack_num=12, filler_num=6)
    _perturb(att)
    att._forward_templates()
    gs = R.params64(att.generator_state(), grad=False)
    out = att.last_forward()
    fw = R.g_forward(gs, att.template_rowptr, att.template_cols, att.template_vals)
    _compare_forward(fw, out["a"], out["cls"], out["value"], att.template_vals, f"{name} templates")
    assert np.abs(out["h1"] - fw["h1"].numpy()).max() <= 1e-6
    assert len(np.unique(out["cls"])) >= 3, "the perturbed boundaries must exercise several classes"
    # one dataset batch of real rows (256 rows, or all users of the small case), through pretrain_G's own path
    np.random.seed(1)
    ep = att.epoch_batches()
    r0, n, k0, ne = ep["batches"][0]
    dev = gpu_device
    f32 = lambda m: torch.zeros(max(1, m), dtype=torch.float32, device=dev)      # noqa: E731
    norm, h1, a, value = f32(n), f32(n * 128), f32(len(ep["col_h"])), f32(len(ep["col_h"]))
    cls = torch.zeros(len(ep["col_h"]), dtype=torch.int32, device=dev)
    att.g_forward(ep["rowptr"][r0:r0 + n + 1], ep["col"], ep["val"], n, norm, h1, a, cls, value)
    rp = ep["rowptr_h"][r0:r0 + n + 1] - k0
    fw = R.g_forward(gs, rp, ep["col_h"][k0:k0 + ne], ep["val_h"][k0:k0 + ne])
    s = slice(k0, k0 + ne)
    _compare_forward(fw, a[s].cpu().numpy(), cls[s].cpu().numpy(), value[s].cpu().numpy(), ep["val_h"][s], f"{name} batch of {n}")


def test_generator_forward_row_lengths(gpu_device):
    """Rows with 1, fewer than filler_num and filler_num entries (and an empty template CSR row does not occur: every user
    of an explicit dataset has a rating); filler_num larger than every row keeps whole rows."""
    ds, mat = _synth(gpu_device)
    att = _att(ds, gpu_device, attack_num=1500, filler_num=6, np_seed=2)      # 1 500 draws of 150 users: every user is a template
    lens = np.diff(att.template_rowptr)
    assert {1, 3, 6} <= set(lens.tolist())
    assert np.array_equal(lens, np.minimum(6, (mat[att.template_users] != 0).sum(1)))
    fw = R.g_forward(R.params64(att.generator_state(), grad=False), att.template_rowptr, att.template_cols, att.template_vals)
    out = att.last_forward()
    _compare_forward(fw, out["a"], out["cls"], out["value"], att.template_vals, "row lengths 1..6")
    big = _att(ds, gpu_device, attack_num=20, filler_num=500)
    assert np.array_equal(np.diff(big.template_rowptr), (mat[big.template_users] != 0).sum(1))
    fake = big.generate_fake(target_id_list=[0])
    assert np.array_equal((fake[:, 1:] != 0), (mat[big.template_users][:, 1:] != 0))


@pytest.mark.parametrize("name", ["synth", "game", "ml1m", "yelp"])
def test_generator_backward_from_dvalue(gpu_device, name):
    ds = _datasets(name, gpu_device)
    att = _att(ds, gpu_device, attack_num=12, filler_num=6)
    _perturb(att)
    att._forward_templates()
    rng = np.random.default_rng(0)
    dv = rng.standard_normal(att.n_fake).astype(np.float32)
    att._backward_templates(torch.as_tensor(dv).to(gpu_device))
    gs = R.params64(att.generator_state())
    fw = R.g_forward(gs, att.template_rowptr, att.template_cols, att.template_vals)
    keep = (fw["margin"].numpy() >= MARGIN)
    assert (~keep).mean() <= 0.01
    (fw["masked"] * torch.as_tensor(dv * keep).to(R.DT)).sum().backward()
    if not keep.all():
        att._backward_templates(torch.as_tensor(dv * keep).to(gpu_device))
    _check_grads(att.generator_grad(), {k: v.grad for k, v in gs.items()}, f"{name} dvalue")
    assert np.abs(gs["min_boundary_value"].grad.numpy()).max() > 0 and np.abs(gs["interval_lengths"].grad.numpy()).max() > 0


@pytest.mark.parametrize("name", ["synth", "game", "ml1m", "yelp"])
def test_pretrain_first_batch_loss_gradient_and_adam(gpu_device, name):
    """pretrain_G's first batch: the CE loss, dL/d(all G parameters) and the Adam step, against the restatement."""
    ds = _datasets(name, gpu_device)
    att = _att(ds, gpu_device, attack_num=12, filler_num=6)
    _perturb(att)
    state0 = att.generator_state()
    perm = np.random.default_rng(4).permutation(att.n_users)[: att.batch_size]        # one batch only
    gs = R.params64(state0)
    ptr, idx, val = att._host_csr
    # the CE is a mean over the batch, so entries near a boundary cannot be left out of the device's loss afterwards: they
    # are taken out of the batch's rows instead (on both sides), until the restatement sees none; at most 1 % in all
    keep = np.ones(len(idx), dtype=bool)
    total = int((ptr[perm + 1] - ptr[perm]).sum())
    for _ in range(64):
        cptr = np.concatenate([[0], np.cumsum(np.add.reduceat(keep, ptr[:-1]) * (np.diff(ptr) > 0))]).astype(np.int64)
        rp, col, x = gather_rows(cptr, idx[keep], val[keep], perm)
        with torch.no_grad():
            near = R.g_forward(gs, rp, col, x)["margin"].numpy() < MARGIN
        if not near.any():
            break
        src = np.flatnonzero(keep)[np.repeat(cptr[perm] - rp[:-1], np.diff(rp)) + np.arange(rp[-1])]
        keep[src[near]] = False
    assert not near.any() and (~keep).sum() <= 0.01 * total
    print(f"{name}: {(~keep).sum()} of {total} entries left out near a boundary")
    att._host_csr = (cptr, idx[keep], val[keep])
    loss = att.pretrain_G(perm=perm)
    fw = R.g_forward(gs, rp, col, x)
    ref = R.ce_loss(fw)
    ref.backward()
    print(f"{name}: CE loss device {loss:.8f} restatement {float(ref):.8f}")
    assert abs(loss - float(ref)) <= LOSS_RTOL * abs(float(ref))
    _check_grads(att.generator_grad(), {k: v.grad for k, v in gs.items()}, f"{name} CE")
    after = att.generator_state()
    for k, v in gs.items():
        g = v.grad.numpy()
        _check_adam(after[k].numpy(), v.detach().numpy(), g, att.lr_g, k)
        assert np.array_equal(after[k].numpy()[g == 0], state0[k].numpy()[g == 0]), k


# ---------------------------------------------------------------- D
@pytest.mark.parametrize("name", ["synth", "game", "ml1m", "yelp"])
def test_discriminator_step(gpu_device, name):
    """train_D's first batch (real rows label 1, fake rows label 0): D's outputs, the loss, every parameter gradient and the
    Adam step; then the adversarial form (fake rows, label 1) with dL/d(input value) at the template entries."""
    ds = _datasets(name, gpu_device)
    att = _att(ds, gpu_device, attack_num=12, filler_num=6)
    _perturb(att)
    state0 = att.discriminator_state()
    perm = np.random.default_rng(4).permutation(att.n_users)[: att.batch_size]
    loss = att.train_D(perm=perm)
    A = att.attack_num
    p_dev = att.d_outputs(2 * A)
    dsr = R.params64(state0)
    rp, col, x = gather_rows(*att._host_csr, perm[:A])
    value = att.last_forward()["value"]
    p_real = R.d_forward(dsr, rp, col, x)
    p_fake = R.d_forward(dsr, att.template_rowptr, att.template_cols, value)
    ref = R.bce(p_real, 1.0) + R.bce(p_fake, 0.0)
    ref.backward()
    print(f"{name}: D loss device {loss:.8f} restatement {float(ref):.8f}")
    assert np.abs(p_dev - torch.cat([p_real, p_fake]).detach().numpy()).max() <= 1e-6
    assert abs(loss - float(ref)) <= LOSS_RTOL * abs(float(ref))
    _check_grads(att.discriminator_grad(), {k: v.grad for k, v in dsr.items()}, f"{name} D")
    after = att.discriminator_state()
    for k, v in dsr.items():
        g = v.grad.numpy()
        _check_adam(after[k].numpy(), v.detach().numpy(), g, att.lr_d, k)
    # adversarial: BCE(D(fake), 1) and its gradient at D's input
    dsr = R.params64(att.discriminator_state(), grad=False)
    v = torch.as_tensor(value).to(R.DT).requires_grad_(True)
    adv = R.bce(R.d_forward(dsr, att.template_rowptr, att.template_cols, v), 1.0)
    adv.backward()
    out = torch.zeros(1, dtype=torch.float32, device=gpu_device)
    att.d_step(0, None, None, None, 1.0, A, 1.0, None, False, att._t_din, out)
    assert abs(float(out.cpu()[0]) - float(adv)) <= LOSS_RTOL * float(adv)
    assert _relerr(att._t_din[: att.n_fake].cpu().numpy(), v.grad.numpy()) <= GRAD_RTOL


def test_adversarial_phase_chain(gpu_device):
    """train_G(adv): BCE(D(G(templates)), 1) through D's input and the projection into every G parameter."""
    ds = _game(gpu_device)
    att = _att(ds, gpu_device, attack_num=12, filler_num=6)
    _perturb(att)
    gs, dsr = R.params64(att.generator_state()), R.params64(att.discriminator_state(), grad=False)
    loss = float(att.train_G_adv().cpu()[0])
    fw = R.g_forward(gs, att.template_rowptr, att.template_cols, att.template_vals)
    assert (fw["margin"].numpy() >= MARGIN).all()
    ref = R.bce(R.d_forward(dsr, att.template_rowptr, att.template_cols, fw["masked"]), 1.0)
    ref.backward()
    assert abs(loss - float(ref)) <= LOSS_RTOL * float(ref)
    _check_grads(att.generator_grad(), {k: v.grad for k, v in gs.items()}, "adv chain")


# ---------------------------------------------------------------- the surrogate phase
def test_surrogate_phase_chain(gpu_device):
    """Phase 4: with the surrogate's X-bar taken from the device, dL/d(all G parameters) against float64 autograd."""
    ds, _ = _synth(gpu_device)
    att = _att(ds, gpu_device)
    _perturb(att)
    gs = R.params64(att.generator_state())
    loss = float(att.train_G_attack([0]).cpu()[0])
    xbar = att.last_hypergradient()
    assert np.isfinite(loss) and np.abs(xbar).max() > 0
    fw = R.g_forward(gs, att.template_rowptr, att.template_cols, att.template_vals)
    keep = fw["margin"].numpy() >= MARGIN
    assert keep.all()
    assert np.array_equal(att.last_forward()["value"], fw["masked"].detach().numpy().astype(np.float32))
    (fw["masked"] * torch.as_tensor(xbar).to(R.DT)).sum().backward()
    _check_grads(att.generator_grad(), {k: v.grad for k, v in gs.items()}, "surrogate chain")


# ---------------------------------------------------------------- whole steps
def test_train_step_contract_and_bit_identity(gpu_device):
    ds, _ = _synth(gpu_device)
    runs = []
    for _ in range(2):
        att = _att(ds, gpu_device, attack_num=10, filler_num=6)
        assert list(att.input_describe()["train_step"]) == ["target_id_list"]
        assert list(att.output_describe()["train_step"]) == ["g_adv", "g_rec"]
        r1 = att.train_step(target_id_list=[0, 5])
        ph1 = dict(att.last_phase_losses)
        r2 = att.train_step(target_id_list=[0, 5])
        assert r1[0] == 0.0 and r2[0] == 0.0 and np.isfinite(r1[1]) and np.isfinite(r2[1])
        assert r2[1] == att.last_phase_losses["attack"][-1]
        assert set(ph1) == {"pretrain_g", "pretrain_d", "gan_d", "gan_g", "attack"} and "pretrain_g" not in att.last_phase_losses
        assert len(ph1["pretrain_g"]) == 1 and len(ph1["pretrain_d"]) == 1 and len(ph1["attack"]) == 2
        fake = att.generate_fake(target_id_list=[0, 5])
        runs.append((att.g_param.cpu().numpy(), att.d_param.cpu().numpy(), fake, r1, r2))
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert np.array_equal(a, b)
    assert runs[0][3:] == runs[1][3:]
    fake = runs[0][2]
    assert fake.shape == (10, ds.n_items) and fake.dtype == np.float32
    assert set(np.unique(fake)) <= {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    assert (fake[:5, 0] == 5).all() and (fake[5:, 5] == 5).all()
    with pytest.raises(ValueError, match="target"):
        att.train_step(target_id_list=[])
    with pytest.raises(ValueError, match="target"):
        att.generate_fake(target_id_list=[ds.n_items])


def test_empty_template_rows_and_refused_target(gpu_device):
    """filler_num 0 gives templates without entries: every phase still runs, the fakes hold the targets only.  A target every
    real user rated is refused by name (the reference's loss is NaN there)."""
    ds, mat = _synth(gpu_device)
    att = _att(ds, gpu_device, filler_num=0)
    assert att.n_fake == 0 and np.array_equal(att.template_rowptr, np.zeros(11, np.int64))
    g_adv, g_rec = att.train_step(target_id_list=[0])
    assert g_adv == 0.0 and np.isfinite(g_rec)
    fake = att.generate_fake(target_id_list=[0])
    expect = np.zeros_like(fake)
    expect[:, 0] = 5
    assert np.array_equal(fake, expect)
    mat2 = mat.copy()
    mat2[:, 1] = 3
    u, i = np.nonzero(mat2)
    ds2 = dataset.from_config("explicit", "all", device=gpu_device, train_dict=np.stack([u, i, mat2[u, i].astype(np.int64)], 1))
    with pytest.raises(ValueError, match="every real user has rated target 1"):
        _att(ds2, gpu_device).train_step(target_id_list=[1])


# ---------------------------------------------------------------- workflows
def _ml1m_data(dev):
    d = synth.make("ml1m")
    victim = dataset.from_config("implicit", "ml1m", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], device=dev,
                                 graph_source="train", seed=5)
    r = synth.with_ratings(d)
    explicit = dataset.from_config("explicit", "ml1m", train_csr=r["train"], valid_csr=r["valid"], test_csr=r["test"], device=dev)
    np.random.seed(7)
    return victim, explicit, explicit.partial_sample(user_ratio=0.2)


def test_no_defense_workflow_with_aushplus(gpu_device):
    victim_data, _, attack_data = _ml1m_data(gpu_device)
    wf = workflow.from_config("no defense", victim_data=victim_data, attack_data=attack_data,
                              victim=model.from_config("victim", "lightgcn", latent_dim_rec=32, lightGCN_n_layers=2),
                              attacker=model.from_config("attacker", "aushplus", device=gpu_device, epoch_s=3, epoch_surrogate=2),
                              rec_epoch=1, attack_epoch=2, target_id_list=[0], device=gpu_device)
    res = wf.execute()
    assert res["n_eval_users"] > 0
    assert all(np.isfinite(v) for v in res.values())
    assert wf.fake_dataset.n_users > victim_data.n_users


def test_defense_workflow_with_aushplus(gpu_device):
    victim_data, explicit, attack_data = _ml1m_data(gpu_device)
    wf = workflow.from_config("defense", victim_data=victim_data, attack_data=attack_data, defense_data=explicit,
                              victim=model.from_config("victim", "lightgcn", latent_dim_rec=32, lightGCN_n_layers=2),
                              attacker=model.from_config("attacker", "aushplus", device=gpu_device, epoch_s=3, epoch_surrogate=2),
                              defender=model.from_config("defender", "PCASelectUsers", device=gpu_device),
                              rec_epoch=1, attack_epoch=1, target_id_list=[0], device=gpu_device)
    res = wf.execute()
    for part in (v for v in res.values() if isinstance(v, dict)):       # the result per stage: HR@K / pred_shift
        assert "pred_shift" in part and any(k.startswith("HR@") for k in part), res
        assert all(np.isfinite(v) for v in part.values()), res
    assert any(isinstance(v, dict) for v in res.values())
    assert wf.defender.user_num == wf.fake_dataset.n_users
    assert res["n_flagged"] == flag_count(50, wf.fake_dataset.n_users) == 50
