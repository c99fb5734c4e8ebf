"""APR victim on MI355X: Adversarial Personalized Ranking (He, He, Du and Chua, SIGIR 2018, "Adversarial Personalized Ranking for
Recommendation"): matrix factorisation under the BPR loss, with a second BPR term evaluated at the embeddings moved by the
worst-case perturbation of size ``eps`` (per row, Delta = eps * Gamma / |Gamma|, Gamma the gradient of the data term).  With
``adv_reg = 0`` it is plain BPR-MF, the usual baseline victim of the poisoning literature (``mf`` is the reference's pointwise BCE
model).

It is not in the reference.  include/recad_hip.h states the exact definition (Gamma and the gradient rows to the bit, in key
order and without float atomics; dots, norms and losses under rounding budgets), csrc/apr.hip computes it, and
tests/_apr_restate.py restates it in numpy.  Given the triplets a step is a deterministic function of the tables: two trainings
from one seed give the same bits.  It is an embedding model: it scores through ``scoring_tables()``, that is through rk_score_topk
and the EvalSession replay, and it holds no I x I matrix.

The tables are ONE [N = U + I, d] parameter ``weight``, users first, drawn as N(0, init_std) from torch's global RNG;
``embedding_user`` / ``embedding_item`` are views of it.  ``train_step`` takes the dataset's pairwise epoch and returns
(mean over the steps of L + adv_reg * L' + R,); ``last_losses`` keeps the three means.

The switch to adversarial training: the epochs before ``adv_start_epoch`` run with adv_reg = 0.  The count is the victim's own
completed ``train_step`` calls, the buffer ``epochs_done``, so ``state_dict()`` carries it; the switch is logged once.  The default
is 200 because the workflows' default rec_epoch is 400 and the paper starts from a trained BPR model.  Adversarial training from the
0.01 initialisation does not train at eps = 0.5: with rows of norm about 0.04 a perturbation of norm 0.5 swamps them (in a float64
run of tests/_apr_restate.py on the tiny set the data loss stayed at 0.693 for 40 epochs and recall@10 was 0.04 against 0.23).

Optimizers: torch.optim.Adam with its default options runs fused in the library, its moments being the entries of
``optimizer.state``; any other optimizer gets the dense gradient of each minibatch from the library and steps in torch.

Groups: ``APR.train_group(victims, epochs)`` trains up to RK_APR_MAX_GROUP victims (fused Adam only) through
rk_apr_train_epoch_group, one launch chain for all of them, each on its own dataset's triplets; every victim ends with the bits its
own ``train_step`` loop would have given it.  ``workflow.Sweep`` retrains its poisoned victims that way."""
import ctypes as C
import math

import torch
import torch.nn as nn

from .. import _lib
from .._ratings import device_refusal
from ..utils import VarDim, get_logger, pick_optim
from .base import BaseVictim


def _f32(x):
    return torch.tensor(float(x), dtype=torch.float32).item()       # what the kernel receives


def _number(x):
    return not isinstance(x, bool) and isinstance(x, (int, float))


def _count(x):
    return not isinstance(x, bool) and isinstance(x, int)


def check_config(factor_num, reg_lambda, eps, adv_reg, adv_start_epoch=0, init_std=0.01, batch=None):
    """The host-side refusals (ValueError), before any device call."""
    if not (_count(factor_num) and 1 <= factor_num <= _lib.RK_APR_MAX_DIM):
        raise ValueError(f"APR: factor_num = {factor_num!r}, expected an integer in 1..{_lib.RK_APR_MAX_DIM}")
    for name, x in (("reg_lambda", reg_lambda), ("eps", eps), ("adv_reg", adv_reg), ("init_std", init_std)):
        if not (_number(x) and math.isfinite(_f32(x)) and _f32(x) >= 0):
            raise ValueError(f"APR: {name} = {x!r}, expected a finite fp32 number >= 0")
    if not (_count(adv_start_epoch) and adv_start_epoch >= 0):
        raise ValueError(f"APR: adv_start_epoch = {adv_start_epoch!r}, expected an integer >= 0")
    if batch is not None and not (_count(batch) and 1 <= batch <= _lib.RK_APR_MAX_BATCH):
        raise ValueError(f"APR: a minibatch of {batch!r} triplets, expected an integer in 1..{_lib.RK_APR_MAX_BATCH}")


class APR(BaseVictim):
    victim_name = "apr"

    def _build(self, factor_num, reg_lambda, eps, adv_reg, adv_start_epoch, init_std, **config):
        self.dataset = config["dataset"]
        self.config = config
        self.logger = get_logger(__name__, config.get("logging_level"))
        info = self.dataset.info_describe()
        self.num_users, self.num_items = int(info["n_users"]), int(info["n_items"])
        check_config(factor_num, reg_lambda, eps, adv_reg, adv_start_epoch, init_std)
        if self.num_users < 1 or self.num_items < 1:
            raise ValueError(f"APR: an empty catalogue ({self.num_users} users x {self.num_items} items)")
        self.dim, self.reg_lambda, self.eps, self.adv_reg = factor_num, float(reg_lambda), float(eps), float(adv_reg)
        self.adv_start_epoch = adv_start_epoch
        self.weight = nn.Parameter(torch.randn(self.num_users + self.num_items, factor_num, dtype=torch.float32) * float(init_std))
        self.register_buffer("epochs_done", torch.zeros(1, dtype=torch.int64))
        self.optimizer = pick_optim(config["optim"])(self.parameters(), lr=config["lr"])
        self._fused_adam = self._adam_is_fused()
        self._ws = None               # the workspace: bytes on the tables' device, as large as the largest epoch so far
        self._grad = None             # dense gradient of the last minibatch (foreign optimizers only)
        self._dummy = None            # moment buffers the library is handed when it is only asked for gradients
        self._adv_logged = False
        self.last_losses = None

    # ------------------------------------------------------------------ the tables
    @property
    def embedding_user(self):
        return self.weight.data[: self.num_users]

    @property
    def embedding_item(self):
        return self.weight.data[self.num_users:]

    def _device(self):
        dev = self.weight.device
        if dev.type != "cuda":
            raise _lib.HipCallError("APR tables are on the CPU: call .to('cuda') first (no CPU fallback)")
        if not self.weight.data.is_contiguous():
            self.weight.data = self.weight.data.contiguous()
        return dev

    def _moments(self, dev):
        """The [N, d] Adam moments: the entries torch.optim.Adam keeps in optimizer.state, re-homed to the tables' device when
        they are not there; zeros the library never updates when the optimizer is a foreign one."""
        if not self._fused_adam:
            if self._dummy is None or self._dummy[0].device != dev:
                self._dummy = (torch.zeros_like(self.weight.data), torch.zeros_like(self.weight.data))
            return self._dummy
        st = self._adam_slot(self.weight)
        for k in ("exp_avg", "exp_avg_sq"):
            if st[k].device != dev or not st[k].is_contiguous():
                st[k] = st[k].to(dev).contiguous()
        return st["exp_avg"], st["exp_avg_sq"]

    def _steps_done(self):
        st = self.optimizer.state.get(self.weight, {})
        return int(st["step"]) if "step" in st else 0

    def _workspace(self, n, batch, dev):
        """a buffer that holds the layout of (n, batch); it only grows, so the short last minibatch of the unfused path and the
        next epoch's first one reuse it"""
        lay = _lib.AprLayout()
        _lib.check(_lib.lib().rk_apr_workspace(self.num_users, self.num_items, self.dim, n, batch, C.byref(lay)), "rk_apr_workspace")
        if self._ws is None or self._ws.device != dev or self._ws.numel() < lay.bytes:
            self._ws = torch.empty(lay.bytes, dtype=torch.uint8, device=dev)
        return self._ws

    # ------------------------------------------------------------------ training
    def _desc(self, n, batch, adv_reg, apply_update, dev):
        """rk_apr_desc of an epoch of n triplets in steps of `batch`: the tables, the moments, the workspace and the optimizer's options"""
        m, v = self._moments(dev)
        if not apply_update and (self._grad is None or self._grad.device != dev):
            self._grad = torch.zeros_like(self.weight.data)
        grp = self.optimizer.param_groups[0]
        b1, b2 = grp.get("betas", (0.9, 0.999))
        ws = self._workspace(n, batch, dev)
        return _lib.AprDesc(
            n_users=self.num_users, n_items=self.num_items, dim=self.dim, table=self.weight.data.data_ptr(), m=m.data_ptr(),
            v=v.data_ptr(), grad=None if apply_update else self._grad.data_ptr(), lam=self.reg_lambda, eps=self.eps, adv_reg=adv_reg,
            lr=float(grp.get("lr", 1e-3)), beta1=float(b1), beta2=float(b2), adam_eps=float(grp.get("eps", 1e-8)),
            workspace=ws.data_ptr(), workspace_bytes=ws.numel())

    def _run_epoch(self, users, pos, neg, batch, adv_reg, apply_update=True):
        """ceil(n / batch) steps in the library -> double [n_steps, 3] = {L, L', R} per step, on the device."""
        check_config(self.dim, self.reg_lambda, self.eps, adv_reg, self.adv_start_epoch, batch=batch)
        dev = self._device()
        _lib.require_gpu()
        if apply_update and not self._fused_adam:
            raise _lib.HipCallError("fused update requested with a non-default optimizer (internal error)")
        n = users.numel()
        if n < 1:
            raise ValueError("APR: an epoch without triplets")
        desc = self._desc(n, batch, adv_reg, apply_update, dev)
        n_steps = (n + batch - 1) // batch
        losses = torch.empty(3 * n_steps, dtype=torch.float64, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        rc = _lib.lib().rk_apr_train_epoch(C.byref(desc), _lib.ptr(users), _lib.ptr(pos), _lib.ptr(neg), n, batch, self._steps_done(),
                                           1 if apply_update else 0, _lib.ptr(losses), _lib.ptr(status), _lib.stream_ptr(dev))
        bad = device_refusal(rc, "rk_apr_train_epoch", status)
        if bad:
            raise ValueError(f"APR: the epoch's triplets break rule {bad[0]} ({_lib.RK_APR_RULES.get(bad[0], '?')}), first in triplet {bad[1]}")
        if apply_update:
            self.optimizer.state[self.weight]["step"] += n_steps
        return losses.view(n_steps, 3)

    def _adv_reg_now(self):
        """adv_reg of the coming epoch: 0 before adv_start_epoch of the victim's own epochs"""
        done = int(self.epochs_done.item())
        if done < self.adv_start_epoch or self.adv_reg == 0.0:
            return 0.0
        if not self._adv_logged:
            self._adv_logged = True
            self.logger.info(f"APR: adversarial training from epoch {done} on (eps = {self.eps}, adv_reg = {self.adv_reg})")
        return self.adv_reg

    def train_step(self, **config):
        """One epoch of pairwise training -> (mean over the steps of L + adv_reg * L' + R,)."""
        self.train()
        pbar = config.get("progress_bar", None)
        check_config(self.dim, self.reg_lambda, self.eps, self.adv_reg, self.adv_start_epoch)     # before the sampler launches
        adv_reg = self._adv_reg_now()
        (users, pos, neg), batch = self._collect_epoch(self.dataset, ("users", "positive_items", "negative_items"))
        check_config(self.dim, self.reg_lambda, self.eps, adv_reg, self.adv_start_epoch, batch=batch)
        dev = self._device()
        users, pos, neg = (t.to(dev).long().contiguous() for t in (users, pos, neg))
        if self._fused_adam:
            per_step = self._run_epoch(users, pos, neg, batch, adv_reg).cpu()
        else:
            rows = []

            def grad_step(cols):
                part = self._run_epoch(*cols, max(cols[0].numel(), 1), adv_reg, apply_update=False)
                rows.append(part[0].cpu())
                return part[0, 0] + adv_reg * part[0, 1] + part[0, 2], {self.weight: self._grad.clone()}

            self._unfused_epoch((users, pos, neg), batch, grad_step)
            per_step = torch.stack(rows)
        loss = self._finish_epoch(per_step, adv_reg)
        if pbar:
            pbar.set_description(f"loss: {loss:.4f}")
        return (loss,)

    def _finish_epoch(self, per_step, adv_reg):
        """what an epoch leaves on the host side: the epoch count, last_losses -> the epoch's loss"""
        self.epochs_done += 1
        mean = per_step.mean(dim=0)
        self.last_losses = {"bpr": float(mean[0]), "adv": float(mean[1]), "reg": float(mean[2])}
        return self.last_losses["bpr"] + adv_reg * self.last_losses["adv"] + self.last_losses["reg"]

    @staticmethod
    def check_group(victims):
        """The host-side refusals of train_group (ValueError), before any device call."""
        victims = list(victims)
        if not victims:
            raise ValueError("APR.train_group: an empty group")
        if len(victims) > _lib.RK_APR_MAX_GROUP:
            raise ValueError(f"APR.train_group: {len(victims)} victims, at most {_lib.RK_APR_MAX_GROUP} train in one group (chunk the list)")
        for r, v in enumerate(victims):
            if not isinstance(v, APR) or not v.__dict__.get("_is_instantiate", False):
                raise ValueError(f"APR.train_group: member {r} is {type(v).__name__}, expected an instantiated APR")
            if any(v is w for w in victims[:r]):
                raise ValueError(f"APR.train_group: member {r} is in the group twice")
            if not v._fused_adam:
                raise ValueError(f"APR.train_group: member {r} has the optimizer {type(v.optimizer).__name__}; a group trains under the fused "
                                 "Adam only (train it with train_step)")
        first = victims[0]
        for r, v in enumerate(victims):
            if v.dim != first.dim:
                raise ValueError(f"APR.train_group: member {r} has factor_num = {v.dim}, member 0 has {first.dim}")
            if v.weight.device != first.weight.device:
                raise ValueError(f"APR.train_group: member {r} is on the device {v.weight.device}, member 0 on {first.weight.device}")
        # the batch size a dataset of this build declares; a foreign dataset's is known once its epoch is drawn (train_group compares again)
        configs = [getattr(v.dataset, "config", None) for v in victims]
        APR._same_batch([c.get("pairwise_batch_size") if isinstance(c, dict) else None for c in configs])
        return victims

    @staticmethod
    def _same_batch(sizes):
        known = [(r, b) for r, b in enumerate(sizes) if b is not None]
        for r, b in known:
            if b != known[0][1]:
                raise ValueError(f"APR.train_group: member {r} trains in minibatches of {b}, member {known[0][0]} in minibatches of {known[0][1]}")

    @staticmethod
    def train_group(victims, epochs=1, progress_bar=None):
        """`epochs` epochs of every victim, each on the triplets of its own dataset, one rk_apr_train_epoch_group call per epoch
        -> [[loss of epoch e for victim r]].  Every victim ends as `epochs` calls of its own train_step() would leave it, to the bit:
        weight, moments, step counter, epochs_done, last_losses, and its dataset's sampler."""
        victims = APR.check_group(victims)
        if not (_count(epochs) and epochs >= 0):
            raise ValueError(f"APR.train_group: epochs = {epochs!r}, expected an integer >= 0")
        R, out = len(victims), []
        for _ in range(epochs):
            adv, cols, sizes = [], [], []
            for v in victims:
                v.train()
                check_config(v.dim, v.reg_lambda, v.eps, v.adv_reg, v.adv_start_epoch)
                adv.append(v._adv_reg_now())
                c, batch = v._collect_epoch(v.dataset, ("users", "positive_items", "negative_items"))
                check_config(v.dim, v.reg_lambda, v.eps, adv[-1], v.adv_start_epoch, batch=batch)
                cols.append(c)
                sizes.append(batch)
            APR._same_batch(sizes)
            batch = sizes[0]
            dev = victims[0]._device()
            _lib.require_gpu()
            descs, ids, losses, ns = (_lib.AprDesc * R)(), [], [], []
            for r, v in enumerate(victims):
                if v._device() != dev:
                    raise ValueError(f"APR.train_group: member {r} is on the device {v.weight.device}, member 0 on {dev}")
                ids.append([t.to(dev).long().contiguous() for t in cols[r]])
                n = ids[r][0].numel()
                if n < 1:
                    raise ValueError(f"APR.train_group: member {r} has an epoch without triplets")
                descs[r] = v._desc(n, batch, adv[r], True, dev)
                ns.append(n)
                losses.append(torch.empty(3 * ((n + batch - 1) // batch), dtype=torch.float64, device=dev))
            status = torch.zeros(2 * R, dtype=torch.int32, device=dev)
            arr = lambda ts: (C.c_void_p * R)(*[t.data_ptr() for t in ts])
            rc = _lib.lib().rk_apr_train_epoch_group(
                R, descs, arr([i[0] for i in ids]), arr([i[1] for i in ids]), arr([i[2] for i in ids]), (C.c_int64 * R)(*ns), batch,
                (C.c_int32 * R)(*[v._steps_done() for v in victims]), 1, arr(losses), _lib.ptr(status), _lib.stream_ptr(dev))
            if rc != 0:
                for r, (rule, t) in enumerate(status.cpu().view(R, 2).tolist()):
                    if rule:
                        raise ValueError(f"APR.train_group: the triplets of member {r} break rule {rule} ({_lib.RK_APR_RULES.get(rule, '?')}), "
                                         f"first in triplet {t}")
                _lib.check(rc, "rk_apr_train_epoch_group")
            row = []
            for r, v in enumerate(victims):
                n_steps = losses[r].numel() // 3
                v.optimizer.state[v.weight]["step"] += n_steps
                row.append((v._finish_epoch(losses[r].view(n_steps, 3).cpu(), adv[r]),))
            if progress_bar:
                progress_bar.set_description("loss: " + " ".join(f"{x[0]:.4f}" for x in row))
            out.append([x[0] for x in row])
        return out

    # ------------------------------------------------------------------ scoring
    def _tables(self):
        self._device()
        U = self.num_users
        return self.weight.data[:U], self.weight.data[U:]

    def forward(self, users, items):
        ue, ie = self._tables()
        n = users.numel()
        out = torch.empty(n, device=ue.device, dtype=torch.float32)
        _lib.check(_lib.lib().rk_pair_scores(
            int(self.dim), _lib.ptr(ue), _lib.ptr(ie), None, None, 0.0, _lib.ptr(users.long().contiguous()),
            _lib.ptr(items.long().contiguous()), n, _lib.ptr(out), 0.0, 0, _lib.stream_ptr(ue.device)), "rk_pair_scores")
        return out

    scoring_tables_static = True   # views of the parameter, no launches: evaluate.EvalSession asks once and keeps them

    def scoring_tables(self):
        """Tables for the dot-product scoring path: zero biases, mean 0.0."""
        ue, ie = self._tables()
        zb = getattr(self, "_zero_bias", None)
        if zb is None or zb.device != ue.device:
            zb = self._zero_bias = torch.zeros(self.num_users + self.num_items, dtype=torch.float32, device=ue.device)
        return ue, ie, zb[: self.num_users], zb[self.num_users:], 0.0

    def scoring_tables_key(self):
        """Storage and shape of the table (evaluate.EvalSession compares it on every run())."""
        return (self.weight.data_ptr(), tuple(self.weight.shape), str(self.weight.device))

    def input_describe(self):
        return {
            "train_step": {
                "users": (torch.int64, (VarDim(comment="batch"))),
                "positive_items": (torch.int64, (VarDim(comment="batch"))),
                "negative_items": (torch.int64, (VarDim(comment="batch"))),
            },
            "forward": {"users": (torch.int64, (VarDim(comment="batch"))), "items": (torch.int64, (VarDim(comment="batch")))},
        }

    def output_describe(self):
        return {
            "train_step": {"loss": (float, [])},
            "forward": {"unnormalized_scores": (torch.float32, [VarDim(comment="batch")])},
        }
