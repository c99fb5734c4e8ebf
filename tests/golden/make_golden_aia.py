#!/usr/bin/env python3
"""Generate tests/golden/aia_*.npz, the fixtures of the AIA attacker, by IMPORTING the reference (gusye1234/recad v0.0.2, a
checkout passed as --reference).  Modelled on make_golden_aush.py; run by hand, CPU only; nothing under tests/ or the product
imports it.  It copies no reference source: it drives the reference's own

    recad.dataset.from_config("explicit", "game") / .partial_sample(user_ratio=0.2)
    recad.model.from_config("attacker", "aia", ...).I(dataset=...) / train_step / generate_fake

and records the draws on the way by wrapping np.random.choice and np.random.shuffle.

`higher` shim.  The reference's fit_adv imports `higher` (aia.py:432), which is not installed here, so this script puts a
small module of its own into sys.modules["higher"].  innerloop_ctx(model, opt) yields
  * fmodel: torch.func.functional_call of `model` over differentiable copies of P and Q;
  * diffopt: step(loss) takes torch.autograd.grad(loss, (P, Q), create_graph=True) and applies Adam with the state copied
    from `opt` (exp_avg, exp_avg_sq, step; the step counter continues), in this arithmetic form:
        g = g + weight_decay * p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;
        p = p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
It is a restatement of higher's DifferentiableAdam, not higher itself; that the two agree cannot be checked here.  While
inside, the shim records theta, m, v and the step at entry and the unrolled epochs' permutations (the np.random.shuffle
results of those epochs).

Cases (torch.manual_seed(SEED) and np.random.seed(SEED) right before .I(); nothing reseeds afterwards):
  aia_game_e3        the game data after partial_sample(0.2) (the kept users of aush_game_partial), epoch_s 3, filler_num 12,
                     target [0], two train_steps
  aia_game_default   the same data, the reference defaults (epoch_s 50, filler_num 36), target [0], one train_step
  aia_small_state    60 users of that data with their items compacted, as a dense train_mat behind info_describe();
                     attack_num 10, filler_num 8, epoch_s 3, target [0], one train_step; theta, m, v and the permutation at the
                     unrolled entry in full, the loss and the full hypergradient
Recorded: the template draws (choice, and the kept columns of each template shuffle), per train_step the fingerprints of the
WMF init and of theta / m / v at the unrolled entry (sum, sum of squares, float64), SAMPLE_ROWS seeded rows of P and Q and
the target's row of Q at the entry, the step counter there, G_loss, the hypergradient and the generator at the template
positions after the step (row-major over (row, ascending column)); generate_fake's nonzeros at the end.  Each file stays
well under 0.5 MB.

Usage:
    python tests/golden/make_golden_aia.py --reference PATH [--scratch DIR]
"""
import argparse
import contextlib
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 2023
PARTIAL_SEED = 11            # aush_game_partial's
SAMPLE_ROWS = 48


def fp(a):
    a = np.asarray(a, dtype=np.float64)
    return np.asarray([a.sum(), (a * a).sum()])


class Rec:
    entry = None
    init = None
    shuffles = []


def install_higher_shim(torch):
    mod = types.ModuleType("higher")

    class FModel:
        def __init__(self, model, params):
            self.model, self.params = model, params

        def __call__(self, *a, **k):
            return torch.func.functional_call(self.model, self.params, a, k)

        def train(self):
            return self

        def eval(self):
            return self

    class DiffOpt:
        def __init__(self, fmodel, opt, names):
            g = opt.param_groups[0]
            self.fmodel, self.names = fmodel, names
            self.lr, (self.b1, self.b2), self.eps, self.wd = g["lr"], g["betas"], g["eps"], g["weight_decay"]
            self.state = {}
            for n, p in zip(names, g["params"]):
                st = opt.state[p]
                self.state[n] = [st["exp_avg"].clone(), st["exp_avg_sq"].clone(), int(st["step"])]

        def step(self, loss):
            ps = [self.fmodel.params[n] for n in self.names]
            grads = torch.autograd.grad(loss, ps, create_graph=True)
            for n, p, g in zip(self.names, ps, grads):
                m, v, t = self.state[n]
                g = g + self.wd * p
                t += 1
                m = self.b1 * m + (1 - self.b1) * g
                v = self.b2 * v + (1 - self.b2) * g * g
                denom = torch.sqrt(v) / np.sqrt(1 - self.b2 ** t) + self.eps
                self.fmodel.params[n] = p - self.lr / (1 - self.b1 ** t) * m / denom
                self.state[n] = [m, v, t]

    @contextlib.contextmanager
    def innerloop_ctx(model, opt):
        g = opt.param_groups[0]["params"]
        byid = {id(p): n for n, p in model.named_parameters()}
        names = [byid[id(p)] for p in g]
        params = {n: p.detach().clone().requires_grad_(True) for n, p in model.named_parameters()}
        fmodel = FModel(model, params)
        diffopt = DiffOpt(fmodel, opt, names)
        Rec.entry = {"P": params["P"].detach().numpy().copy(), "Q": params["Q"].detach().numpy().copy(),
                     "mP": diffopt.state["P"][0].numpy().copy(), "mQ": diffopt.state["Q"][0].numpy().copy(),
                     "vP": diffopt.state["P"][1].numpy().copy(), "vQ": diffopt.state["Q"][1].numpy().copy(),
                     "step": diffopt.state["P"][2], "n_shuffles_before": len(Rec.shuffles)}
        yield fmodel, diffopt

    mod.innerloop_ctx = innerloop_ctx
    sys.modules["higher"] = mod


@contextlib.contextmanager
def recording():
    real_choice, real_shuffle = np.random.choice, np.random.shuffle
    choices = []

    def choice(*a, **kw):
        out = real_choice(*a, **kw)
        choices.append(np.asarray(out).copy())
        return out

    def shuffle(x):
        real_shuffle(x)
        Rec.shuffles.append(np.asarray(x).copy())

    np.random.choice, np.random.shuffle = choice, shuffle
    try:
        yield choices
    finally:
        np.random.choice, np.random.shuffle = real_choice, real_shuffle


def run_case(recad, torch, ds, tag, steps, full_state=False, **cfg):
    aia_mod = sys.modules["recad.model.attacker.aia"]
    real_init = aia_mod.WeightedMF.__init__

    def init(self, *a, **k):
        real_init(self, *a, **k)
        Rec.init = (self.P.detach().numpy().copy(), self.Q.detach().numpy().copy())

    aia_mod.WeightedMF.__init__ = init
    info = ds.info_describe()
    mat = np.asarray(info["train_mat"], dtype=np.float32)
    U, I = mat.shape
    targets = [0]
    out = {"n_users": np.int64(U), "n_items": np.int64(I), "seed": np.int64(SEED), "targets": np.asarray(targets, np.int64),
           "steps": np.int64(steps)}
    nz = mat != 0
    out["csr_fp"] = np.asarray([nz.sum(), np.nonzero(nz)[1].astype(np.float64).sum(), mat.astype(np.float64).sum()])
    for k, v in cfg.items():
        out["cfg_" + k] = np.asarray(v)
    try:
        Rec.shuffles = []
        np.random.seed(SEED)
        torch.manual_seed(SEED)
        with recording() as choices:
            att = recad.model.from_config("attacker", "aia", device="cpu", **cfg).I(dataset=ds)
            A, F = att.attack_num, att.filler_num
            out["template_users"] = np.asarray(choices[0], np.int64)
            out["template_cols_drawn"] = np.asarray([s[:F] for s in Rec.shuffles[:A]], np.int64).reshape(A, F)
            mask = (att.real_template > 0).numpy()
            rows, cols = np.nonzero(mask)
            out["pos_rows"], out["pos_cols"] = rows.astype(np.int32), cols.astype(np.int32)
            res = {k: [] for k in ("g_loss", "init_fp", "entry_fp", "entry_step", "entry_P_rows", "entry_Q_rows", "entry_Q_target",
                                   "xbar", "gen")}
            rs = np.random.RandomState(SEED)
            prow = np.sort(rs.choice(U + A, min(SAMPLE_ROWS, U + A), replace=False))
            qrow = np.sort(rs.choice(I, min(SAMPLE_ROWS, I), replace=False))
            out["sample_P"], out["sample_Q"] = prow, qrow
            for s in range(steps):
                (g_loss,) = att.train_step(target_id_list=targets)
                e = Rec.entry
                res["g_loss"].append(g_loss)
                res["init_fp"].append(np.concatenate([fp(Rec.init[0]), fp(Rec.init[1])]))
                res["entry_fp"].append(np.concatenate([fp(e[k]) for k in ("P", "Q", "mP", "mQ", "vP", "vQ")]))
                res["entry_step"].append(e["step"])
                res["entry_P_rows"].append(e["P"][prow])
                res["entry_Q_rows"].append(e["Q"][qrow])
                res["entry_Q_target"].append(e["Q"][targets[0]])
                res["xbar"].append(att.netG.fake_parameter.grad.detach().numpy()[rows, cols])
                res["gen"].append(att.netG.fake_parameter.detach().numpy()[rows, cols])
                if full_state and s == 0:
                    for k in ("P", "Q", "mP", "mQ", "vP", "vQ"):
                        out["state_" + k] = e[k]
                    out["state_perms"] = np.asarray(Rec.shuffles[e["n_shuffles_before"]:], np.int32)
                    out["state_gen"] = att.real_template.numpy()[rows, cols]
            for k, v in res.items():
                out[k] = np.asarray(v)
            fake = att.generate_fake(target_id_list=targets)
            fr, fc = np.nonzero(fake)
            out["fake_rows"], out["fake_cols"], out["fake_vals"] = fr.astype(np.int32), fc.astype(np.int32), fake[fr, fc].astype(np.float32)
    finally:
        aia_mod.WeightedMF.__init__ = real_init
    path = os.path.join(OUT, f"aia_{tag}.npz")
    np.savez_compressed(path, **out)
    print(tag, "G_loss", out["g_loss"], "bytes", os.path.getsize(path))


class DenseData:
    """A dataset with the reference's info_describe() keys the attacker reads (aia.py:44-48)."""

    def __init__(self, mat):
        self.mat = mat

    def info_describe(self):
        return {"n_users": self.mat.shape[0], "n_items": self.mat.shape[1], "train_mat": self.mat}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "recad_golden_scratch"))
    args = ap.parse_args()
    ref_root = os.path.abspath(args.reference)
    os.makedirs(os.path.join(args.scratch, "data"), exist_ok=True)
    if not os.path.exists(os.path.join(args.scratch, "data", "game")):
        with zipfile.ZipFile(os.path.join(ref_root, "data", "game.zip")) as z:
            z.extractall(os.path.join(args.scratch, "data"))
    os.chdir(args.scratch)
    sys.path.insert(0, ref_root)
    import torch

    torch.set_num_threads(4)
    install_higher_shim(torch)
    import recad
    import recad.model.attacker.aia  # noqa: F401

    recad.utils.TQDM = False
    ds = recad.dataset.from_config("explicit", "game")
    np.random.seed(PARTIAL_SEED)
    p = ds.partial_sample(user_ratio=0.2)
    run_case(recad, torch, p, "game_e3", 2, epoch_s=3, filler_num=12)
    run_case(recad, torch, p, "game_default", 1)
    mat = np.asarray(p.info_describe()["train_mat"], dtype=np.float32)[:60]
    used = np.nonzero((mat != 0).any(0))[0]
    small = mat[:, used]
    small_ds = DenseData(small)
    run_case(recad, torch, small_ds, "small_state", 1, full_state=True, attack_num=10, filler_num=8, epoch_s=3)
    d = dict(np.load(os.path.join(OUT, "aia_small_state.npz")))
    nz = small != 0
    ptr = np.zeros(small.shape[0] + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(nz.sum(1))
    d.update(small_ptr=ptr, small_idx=np.nonzero(nz)[1].astype(np.int32), small_val=small[nz], small_items=used.astype(np.int32))
    np.savez_compressed(os.path.join(OUT, "aia_small_state.npz"), **d)


if __name__ == "__main__":
    main()
