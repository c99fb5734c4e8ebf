"""AUSH attacker on the device (recad/model/attacker/aush.py, registry recad/default.py:159-168).

The reference slices dense B x I batches out of a dense U x I train_mat and runs its generator and discriminator as
dense GEMMs.  Here every attack row is the sparse set "fillers U S" of the rating CSR, and csrc/aush.hip does the work:
eligible users, permutation, filler draws, ZR masks, the generator at S, the discriminator's forward / backward /
Adam and generate_fake's assembly.  An epoch reads back only its per-batch losses, once, at the end.

Behaviour kept from the reference, quirks included:
  * the generator never trains: ``gen_output = self.netG(input_template).detach()`` (aush.py:138) cuts it out of every
    loss, so G stays at its initialisation and only D learns; train_step still returns the four losses;
  * in training target_patch is written at selected_ids (aush.py:121), in generate_fake at the targets (aush.py:199);
  * both MSE losses divide by B * n_items (nn.MSELoss over the full B x I arrays, aush.py:162-167);
  * the ZR mask keeps len - floor(len * (1 - ZR_ratio)) of the zero-rated S entries of a batch (aush.py:114-119);
  * generate_fake rates EVERY target 5 on EVERY row (aush.py:199), and rounds half to even at S (aush.py:201-205).
The random draws are this build's own (rk_mix64 keyed on seed, epoch, row and draw): the same distributions as the
reference's np.random calls, not the same numbers.  replay_batch / replay_fake take the reference's draws instead.
"""
import numpy as np
import torch
from torch import nn

from .. import _lib
from ..utils import VarDim
from ..victim.base import BaseVictim
from ._common import open_build

HG, HD = _lib.RK_AUSH_HG, _lib.RK_AUSH_HD
_FAKE_STREAM = 1 << 62


def init_weights(n_items):
    """The reference's initial weights, drawn from torch's CPU RNG in its construction order (aush.py:26-36):
    AushGenerator = Linear(I, 128), Linear(128, I); AushDiscriminator = Linear(I, 150), Linear(150, 150) x 2, Linear(150, 1).
    Returns (generator state, discriminator state) in the reference's nn.Sequential names."""
    g = [nn.Linear(n_items, HG), nn.Linear(HG, n_items)]
    d = [nn.Linear(n_items, HD), nn.Linear(HD, HD), nn.Linear(HD, HD), nn.Linear(HD, 1)]
    gs, ds = {}, {}
    for k, lin in zip((0, 2), g):
        gs[f"main.{k}.weight"], gs[f"main.{k}.bias"] = lin.weight.detach(), lin.bias.detach()
    for k, lin in zip((0, 2, 4, 6), d):
        ds[f"main.{k}.weight"], ds[f"main.{k}.bias"] = lin.weight.detach(), lin.bias.detach()
    return gs, ds


def d_offsets(n_items):
    """Offsets of the packed discriminator (rk_aush_desc.d_param): W1 item-major [I, 150], b1, W2 [150, 150], b2, W3, b3,
    w4 [150], b4 [1]."""
    o = {"main.0.weight": 0}
    o["main.0.bias"] = n_items * HD
    o["main.2.weight"] = o["main.0.bias"] + HD
    o["main.2.bias"] = o["main.2.weight"] + HD * HD
    o["main.4.weight"] = o["main.2.bias"] + HD
    o["main.4.bias"] = o["main.4.weight"] + HD * HD
    o["main.6.weight"] = o["main.4.bias"] + HD
    o["main.6.bias"] = o["main.6.weight"] + HD
    o["end"] = o["main.6.bias"] + 1
    return o


class Aush(BaseVictim):
    """``model.from_config("attacker", "aush", **kw)`` keeps the configuration, ``.I(dataset=explicit)`` builds it,
    ``train_step(target_id_list=...)`` runs one epoch and returns (d_loss, g_loss_rec, g_loss_shilling, g_loss_gan) as the
    float64 means of the per-batch values, ``generate_fake(target_id_list=...)`` returns an attack_num x n_items float32
    array."""

    victim_name = "aush"
    scope = "attacker"

    def _build(self, attack_num, filler_num, lr_g, lr_d, optim_g, optim_d, selected_ids, ZR_ratio, seed, **config):
        ds, U, I, ptr, idx, val = open_build(self, config)
        if str(optim_d).lower() != "adam":
            raise ValueError(f"Aush: optim_d {optim_d!r} is not supported on the device (the reference's default 'adam' is)")
        self.dataset = ds
        self.attack_num, self.filler_num = int(attack_num), int(filler_num)
        self.selected_ids = list(selected_ids)
        self.ZR_ratio, self.lr_d, self.lr_g = float(ZR_ratio), float(lr_d), float(lr_g)
        self.seed = int(np.random.randint(0, 2 ** 31 - 1) if seed is None else seed)
        self.n_users, self.n_items = U, I
        self.batch_size = int(getattr(ds, "config", {}).get("batch_size", 256))
        sel = sorted(set(int(s) for s in self.selected_ids))
        if not sel or sel[0] < 0 or sel[-1] >= I or len(sel) > _lib.RK_AUSH_MAX_SELECT:
            raise ValueError(f"Aush: selected_ids must be 1..{_lib.RK_AUSH_MAX_SELECT} item ids in [0, {I})")
        if not 0 < self.filler_num <= _lib.RK_AUSH_MAX_FILLER:
            raise ValueError(f"Aush: filler_num must be in [1, {_lib.RK_AUSH_MAX_FILLER}]")
        if self.batch_size * len(sel) > _lib.RK_AUSH_MAX_PAIRS:
            raise ValueError(f"Aush: batch_size * |selected_ids| must be at most {_lib.RK_AUSH_MAX_PAIRS}")
        dev = self.device
        self._sel_host = np.asarray(sel, dtype=np.int32)
        self._sel = torch.as_tensor(self._sel_host).to(dev)
        self._rowptr = torch.as_tensor(np.asarray(ptr).astype(np.int32)).to(dev)
        self._col = torch.as_tensor(np.asarray(idx).astype(np.int32)).to(dev)
        self._val = torch.as_tensor(np.asarray(val).astype(np.float32)).to(dev)
        gs, dstate = init_weights(I)
        self.g_w1t = gs["main.0.weight"].t().contiguous().to(dev)
        self.g_b1 = gs["main.0.bias"].contiguous().to(dev)
        self.g_w2 = gs["main.2.weight"].contiguous().to(dev)
        self.g_b2 = gs["main.2.bias"].contiguous().to(dev)
        o = d_offsets(I)
        packed = torch.empty(o["end"], dtype=torch.float32)
        packed[: o["main.0.bias"]] = dstate["main.0.weight"].t().reshape(-1)
        for k in ("main.0.bias", "main.2.weight", "main.2.bias", "main.4.weight", "main.4.bias", "main.6.weight", "main.6.bias"):
            v = dstate[k].reshape(-1)
            packed[o[k]:o[k] + v.numel()] = v
        self.d_param = packed.to(dev)
        self.d_m = torch.zeros_like(self.d_param)
        self.d_v = torch.zeros_like(self.d_param)
        self._touched = torch.zeros(I, dtype=torch.uint8, device=dev)
        self._touched_list = torch.zeros(I, dtype=torch.int32, device=dev)
        self._n_touched = torch.zeros(1, dtype=torch.int32, device=dev)
        self._gslot = torch.full((I,), -1, dtype=torch.int32, device=dev)
        nb = _lib.C.c_int64()
        L = _lib.lib()
        _lib.check(L.rk_aush_workspace_bytes(self.batch_size, self.filler_num, len(sel), _lib.C.byref(nb)), "rk_aush_workspace_bytes")
        self._work = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
        d = _lib.AushDesc()
        d.n_users, d.n_items, d.filler_num, d.n_sel, d.batch = U, I, self.filler_num, len(sel), self.batch_size
        for f, t in (("rowptr", self._rowptr), ("col", self._col), ("val", self._val), ("sel", self._sel), ("g_w1t", self.g_w1t),
                     ("g_b1", self.g_b1), ("g_w2", self.g_w2), ("g_b2", self.g_b2), ("d_param", self.d_param), ("d_m", self.d_m),
                     ("d_v", self.d_v), ("touched", self._touched), ("touched_list", self._touched_list),
                     ("n_touched", self._n_touched), ("gslot", self._gslot), ("work", self._work)):
            setattr(d, f, t.data_ptr())
        d.work_bytes = int(nb.value)
        d.lr, d.beta1, d.beta2, d.eps = self.lr_d, 0.9, 0.999, 1e-8   # torch.optim.Adam defaults (utils.py:181-183)
        self._desc = d
        self._pools = {}
        self._epoch = 0
        self._adam_t = 0
        self._fake_calls = 0
        self.last_batch_losses = None
        self.last_fake = None

    # ------------------------------------------------------------------ description (aush.py:46-58)
    def forward(self):
        pass

    def input_describe(self):
        return {"train_step": {"target_id_list": (list, VarDim())}}

    def output_describe(self):
        return {"train_step": {"d_losses": (float, []), "g_loss_rec_l": (float, []), "g_loss_shilling_l": (float, []),
                               "g_loss_gan_l": (float, [])}}

    # ------------------------------------------------------------------ parameters in the reference's layout
    def generator_state(self):
        """netG.state_dict() of the reference (CPU tensors)."""
        return {"main.0.weight": self.g_w1t.t().cpu().contiguous(), "main.0.bias": self.g_b1.cpu(),
                "main.2.weight": self.g_w2.cpu(), "main.2.bias": self.g_b2.cpu()}

    def discriminator_state(self):
        """netD.state_dict() of the reference (CPU tensors), unpacked from the device buffer."""
        o = d_offsets(self.n_items)
        p = self.d_param.cpu()
        shapes = {"main.0.bias": (HD,), "main.2.weight": (HD, HD), "main.2.bias": (HD,), "main.4.weight": (HD, HD),
                  "main.4.bias": (HD,), "main.6.weight": (1, HD), "main.6.bias": (1,)}
        out = {"main.0.weight": p[: o["main.0.bias"]].view(self.n_items, HD).t().contiguous()}
        for k, sh in shapes.items():
            n = int(np.prod(sh))
            out[k] = p[o[k]:o[k] + n].view(*sh).clone()
        return out

    # ------------------------------------------------------------------ plumbing
    def _pool(self, target_id_list):
        """Filler pool and eligible users for S U T (cached per target set)."""
        key = tuple(sorted(set(int(t) for t in target_id_list)))
        if key in self._pools:
            return self._pools[key]
        if key and (key[0] < 0 or key[-1] >= self.n_items):
            raise ValueError(f"Aush: target ids must lie in [0, {self.n_items})")
        dev, L, P = self.device, _lib.lib(), _lib.ptr
        excl = torch.as_tensor(np.asarray(sorted(set(key) | set(self._sel_host.tolist())), dtype=np.int32)).to(dev)
        pool_ptr = torch.empty(self.n_users + 1, dtype=torch.int32, device=dev)
        pool_col = torch.empty(max(1, self._col.numel()), dtype=torch.int32, device=dev)
        eligible = torch.empty(self.n_users, dtype=torch.int32, device=dev)
        n = _lib.C.c_int32()
        _lib.check(L.rk_aush_eligible(self.n_users, P(self._rowptr), P(self._col), P(self._val), P(excl), excl.numel(), self.filler_num,
                                      P(pool_ptr), P(pool_col), P(eligible), _lib.C.byref(n), _lib.stream_ptr(dev)), "rk_aush_eligible")
        pool = {"ptr": pool_ptr, "col": pool_col, "eligible": eligible[: n.value], "n": int(n.value),
                "targets": torch.as_tensor(np.asarray(key, dtype=np.int32)).to(dev), "key": key}
        self._pools[key] = pool
        return pool

    def _rows(self, n):
        dev, F, S = self.device, self.filler_num, len(self._sel_host)
        return {"fcol": torch.empty(n * F, dtype=torch.int32, device=dev), "fval": torch.empty(n * F, dtype=torch.float32, device=dev),
                "nf": torch.empty(n, dtype=torch.int32, device=dev), "sval": torch.empty(n * S, dtype=torch.float32, device=dev),
                "gen": torch.empty(n * S, dtype=torch.float32, device=dev), "zr": torch.empty(n * S, dtype=torch.uint8, device=dev)}

    def _sample(self, users, rows, pool=None, draws=None, stream_id=0):
        L, P, n = _lib.lib(), _lib.ptr, int(users.numel())
        _lib.check(L.rk_aush_sample(n, P(users), self.filler_num, P(self._rowptr), P(self._col), P(self._val),
                                    P(pool["ptr"]) if pool else None, P(pool["col"]) if pool else None, P(draws), self.seed, stream_id, 0,
                                    P(self._sel), len(self._sel_host), P(rows["fcol"]), P(rows["fval"]), P(rows["nf"]), P(rows["sval"]),
                                    _lib.stream_ptr(self.device)), "rk_aush_sample")
        _lib.check(L.rk_aush_gen(n, self.filler_num, P(rows["fcol"]), P(rows["fval"]), P(rows["nf"]), P(self.g_w1t), P(self.g_b1),
                                 P(self.g_w2), P(self.g_b2), P(self._sel), len(self._sel_host), P(rows["gen"]), _lib.stream_ptr(self.device)),
                   "rk_aush_gen")

    def _as_dev_i32(self, a, bound, what):
        a = np.asarray(a)
        if a.size and (int(a.min()) < 0 or int(a.max()) >= bound):
            raise ValueError(f"Aush: {what} must lie in [0, {bound})")
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

    # ------------------------------------------------------------------ aush.py:79-175
    def train_step(self, **config):
        """One epoch over the eligible users (a fresh permutation, batches of batch_size, the last one short)."""
        pool = self._pool(config["target_id_list"])
        N = pool["n"]
        if N == 0:
            raise ValueError(f"Aush.train_step: no user has {self.filler_num} rated items outside selected_ids and the targets")
        if pool.get("rows_n") != N:
            pool["rows"] = self._rows(N)
            pool["perm"] = torch.empty(N, dtype=torch.int32, device=self.device)
            pool["rows_n"] = N
        nb = (N + self.batch_size - 1) // self.batch_size
        losses = torch.empty(nb * 4, dtype=torch.float32, device=self.device)
        r, P = pool["rows"], _lib.ptr
        _lib.check(_lib.lib().rk_aush_train_epoch(_lib.C.byref(self._desc), P(pool["eligible"]), N, P(pool["ptr"]), P(pool["col"]), self.seed,
                                                  self._epoch, self.ZR_ratio, self._adam_t, P(pool["perm"]), P(r["fcol"]), P(r["fval"]),
                                                  P(r["nf"]), P(r["sval"]), P(r["gen"]), P(r["zr"]), P(losses),
                                                  _lib.stream_ptr(self.device)), "rk_aush_train_epoch")
        self._epoch += 1
        self._adam_t += nb
        out = losses.cpu().numpy().reshape(nb, 4).astype(np.float64)     # the epoch's one read-back
        self.last_batch_losses = out
        return tuple(float(x) for x in out.mean(axis=0))

    def replay_batch(self, users, draws, zr, target_id_list=None):
        """One train_step batch on a given sample: users [B], the filler draws [B, filler_num] (item ids, with repeats) and the
        ZR ones [B, |S|] (columns in ascending item order).  Returns (d_loss, g_loss_rec, g_loss_shilling, g_loss_gan) and
        advances D's Adam step like a batch of train_step."""
        users = self._as_dev_i32(users, self.n_users, "user ids")
        B = int(users.numel())
        if not 0 < B <= self.batch_size:
            raise ValueError(f"replay_batch: {B} rows, batch size {self.batch_size}")
        draws = self._as_dev_i32(np.asarray(draws).reshape(B, self.filler_num), self.n_items, "filler draws")
        zr = torch.as_tensor(np.ascontiguousarray(np.asarray(zr).reshape(B, len(self._sel_host)), dtype=np.uint8)).to(self.device)
        rows = self._rows(B)
        self._sample(users, rows, draws=draws)
        losses = torch.empty(4, dtype=torch.float32, device=self.device)
        P = _lib.ptr
        _lib.check(_lib.lib().rk_aush_d_step(_lib.C.byref(self._desc), B, P(rows["fcol"]), P(rows["fval"]), P(rows["nf"]), P(rows["sval"]),
                                             P(rows["gen"]), P(zr.view(-1)), self._adam_t + 1, P(losses), _lib.stream_ptr(self.device)),
                   "rk_aush_d_step")
        self._adam_t += 1
        return tuple(float(x) for x in losses.cpu().numpy())

    # ------------------------------------------------------------------ aush.py:176-208
    def _fake(self, users, rows, pool, n):
        out = torch.empty(n, self.n_items, dtype=torch.float32, device=self.device)
        pre = torch.empty(n * len(self._sel_host), dtype=torch.float32, device=self.device)
        P = _lib.ptr
        tg = pool["targets"]
        _lib.check(_lib.lib().rk_aush_fake_assemble(n, self.n_items, self.filler_num, P(rows["fcol"]), P(rows["fval"]), P(rows["nf"]),
                                                    P(self._sel), len(self._sel_host), P(rows["gen"]), P(tg) if tg.numel() else None,
                                                    tg.numel(), P(pre), P(out), _lib.stream_ptr(self.device)), "rk_aush_fake_assemble")
        self.last_fake = {"users": users.cpu().numpy(), "pre": pre.cpu().numpy().reshape(n, -1), "selected": self._sel_host.copy()}
        return out.cpu().numpy()

    def generate_fake(self, **kwargs):
        """attack_num rows: eligible users permuted, then picked with replacement; fillers drawn; 5 at every target; the
        generator's values at S rounded half to even and clipped to [1, 5]."""
        pool = self._pool(kwargs["target_id_list"])
        if pool["n"] == 0:
            raise ValueError(f"Aush.generate_fake: no user has {self.filler_num} rated items outside selected_ids and the targets")
        call = self._fake_calls
        self._fake_calls += 1
        stream = _FAKE_STREAM | call
        perm = torch.empty(pool["n"], dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().rk_aush_permute(pool["n"], _lib.ptr(pool["eligible"]), self.seed, stream, _lib.ptr(perm),
                                              _lib.stream_ptr(self.device)), "rk_aush_permute")
        pick = np.random.default_rng([self.seed, call]).integers(0, pool["n"], self.attack_num)
        users = perm[torch.as_tensor(pick).to(self.device)].contiguous()
        rows = self._rows(self.attack_num)
        self._sample(users, rows, pool=pool, stream_id=stream)
        return self._fake(users, rows, pool, self.attack_num)

    def replay_fake(self, users, draws, target_id_list):
        """generate_fake on given users [n] and filler draws [n, filler_num] (item ids)."""
        pool = self._pool(target_id_list)
        users = self._as_dev_i32(users, self.n_users, "user ids")
        n = int(users.numel())
        rows = self._rows(n)
        self._sample(users, rows, draws=self._as_dev_i32(np.asarray(draws).reshape(n, self.filler_num), self.n_items, "filler draws"))
        return self._fake(users, rows, pool, n)

    def eligible_users(self, target_id_list):
        """The eligible user ids (ascending) for these targets."""
        return self._pool(target_id_list)["eligible"].cpu().numpy()


class RandomAttacker(BaseVictim):
    """``model.from_config("attacker", "random")``: ``.I(dataset=explicit)`` builds workflow.RandomAttack with the dataset's
    n_items and the mean and population std of its train ratings (heuristic.py:12-17)."""

    victim_name = "random"
    scope = "attacker"

    def I(self, **kwargs):
        from ..workflow import RandomAttack

        config = dict(self._pending)
        config.update(kwargs)
        ds = config.get("dataset")
        if ds is None:
            raise ValueError("the random attacker needs dataset= at .I()")
        info = ds.info_describe()
        r = np.asarray(info["train_kvr"])[:, 2].astype(np.float64)
        return RandomAttack(int(info["n_items"]), attack_num=int(config["attack_num"]), filler_num=int(config["filler_num"]),
                            rating_mean=float(np.mean(r)), rating_std=float(np.std(r)))
