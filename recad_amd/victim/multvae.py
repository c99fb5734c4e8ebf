"""Mult-VAE victim on MI355X: the variational autoencoder with a multinomial likelihood over the whole catalogue (Liang,
Krishnan, Hoffman and Jebara, WWW 2018, "Variational Autoencoders for Collaborative Filtering"): a user's row of the implicit
matrix, L2-normalised and under input dropout, goes through I -> hidden -> (mu, logvar) -> hidden -> I with tanh units, and the
loss is the negative multinomial log-likelihood of the row plus beta times the KL term, beta annealed from 0 to ``anneal_cap``
over ``total_anneal_steps`` updates.

It is not in the reference.  include/recad_hip.h states the exact definition (the sparse layer, every product, the bias sums
and the input layer's gradient to the bit, in a fixed order and without float atomics; tanh, the sample, the KL term and the
row log-softmax under rounding budgets), csrc/multvae.hip computes it, and tests/_multvae_restate.py restates it in numpy.  The
model has no per-user parameters: an injected profile moves a target item only through the shared weights.  Given the order of
the users a step is a deterministic function of the parameters, the seed and the step count: two trainings from one seed give
the same bits.

All parameters are ONE flat fp32 parameter ``theta`` (W1 [I, H], b1, W2 [2L, H], b2, W3 [H, L], b3, W4 [I, H], b4 in this order;
``W1`` ... ``b4`` are views of it), Xavier-normal weights and N(0, 0.001) biases drawn on the host at ``.I()`` from ``seed``
(None: drawn from torch's global RNG).  ``train_step`` is one epoch over a ``torch.randperm`` (global RNG) of the users with at
least one train item and returns (mean step loss,); ``last_losses`` keeps the mean nll and KL.  ``steps_done`` counts the
updates (it drives beta, the dropout masks and the noise) and is part of ``state_dict()``.

Optimizers: torch.optim.Adam with its default options runs fused in the library, its moments being the entries of
``optimizer.state``; any other optimizer gets the flat gradient of each minibatch from the library and steps in torch."""
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


def check_config(hidden_dim, latent_dim, dropout, anneal_cap, total_anneal_steps, batch_size, seed=None):
    """The host-side refusals (ValueError), before any device call."""
    for name, x, hi in (("hidden_dim", hidden_dim, _lib.RK_MVAE_MAX_HIDDEN), ("latent_dim", latent_dim, _lib.RK_MVAE_MAX_LATENT),
                        ("batch_size", batch_size, _lib.RK_MVAE_MAX_BATCH)):
        if not (_count(x) and 1 <= x <= hi):
            raise ValueError(f"Mult-VAE: {name} = {x!r}, expected an integer in 1..{hi}")
    if not (_number(dropout) and 0 <= _f32(dropout) < 1):
        raise ValueError(f"Mult-VAE: dropout = {dropout!r}, expected a number in [0, 1)")
    if not (_number(anneal_cap) and math.isfinite(_f32(anneal_cap)) and _f32(anneal_cap) >= 0):
        raise ValueError(f"Mult-VAE: anneal_cap = {anneal_cap!r}, expected a finite fp32 number >= 0")
    if not (_count(total_anneal_steps) and 0 <= total_anneal_steps < 2 ** 62):
        raise ValueError(f"Mult-VAE: total_anneal_steps = {total_anneal_steps!r}, expected an integer >= 0")
    if seed is not None and not (_count(seed) and 0 <= seed < 2 ** 63):
        raise ValueError(f"Mult-VAE: seed = {seed!r}, expected None or an integer in 0..2^63 - 1")


def beta_at(step, anneal_cap, total_anneal_steps):
    """beta of the update that follows `step` completed ones (the library forms the same double)"""
    cap = _f32(anneal_cap)
    return min(cap, step / total_anneal_steps) if total_anneal_steps > 0 else cap


def param_shapes(n_items, hidden, latent):
    """(name, shape) in the flat buffer's order"""
    I, H, L = n_items, hidden, latent
    return (("W1", (I, H)), ("b1", (H,)), ("W2", (2 * L, H)), ("b2", (2 * L,)), ("W3", (H, L)), ("b3", (H,)), ("W4", (I, H)), ("b4", (I,)))


def init_flat(n_items, hidden, latent, seed):
    """Xavier-normal weights (std = sqrt(2 / (fan_in + fan_out))) and N(0, 0.001) biases, drawn in the buffer's order."""
    gen = torch.Generator().manual_seed(seed)
    fans = {"W1": (n_items, hidden), "W2": (hidden, 2 * latent), "W3": (latent, hidden), "W4": (hidden, n_items)}
    parts = []
    for name, shape in param_shapes(n_items, hidden, latent):
        std = math.sqrt(2.0 / sum(fans[name])) if name in fans else 0.001
        parts.append((torch.randn(shape, generator=gen, dtype=torch.float32) * std).reshape(-1))
    return torch.cat(parts)


class MultVAE(BaseVictim):
    victim_name = "multvae"

    def _build(self, hidden_dim, latent_dim, dropout, anneal_cap, total_anneal_steps, batch_size, seed, **config):
        self.dataset = config["dataset"]
        self.config = config
        self.logger = get_logger(__name__, config.get("logging_level"))
        info = self.dataset.info_describe()
        self.num_users, self.num_items = int(info["n_users"]), int(info["n_items"])
        check_config(hidden_dim, latent_dim, dropout, anneal_cap, total_anneal_steps, batch_size, seed)
        if self.num_users < 1 or not 1 <= self.num_items <= _lib.RK_MVAE_MAX_ITEMS:
            raise ValueError(f"Mult-VAE: {self.num_users} users x {self.num_items} items, expected a catalogue of 1..{_lib.RK_MVAE_MAX_ITEMS}")
        self.hidden, self.latent, self.dropout, self.anneal_cap = hidden_dim, latent_dim, float(dropout), float(anneal_cap)
        self.total_anneal_steps, self.batch_size = total_anneal_steps, batch_size
        self.seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else seed     # from the global RNG, at .I()
        self._slices, at = {}, 0
        for name, shape in param_shapes(self.num_items, hidden_dim, latent_dim):
            self._slices[name] = (at, at + math.prod(shape), shape)
            at += math.prod(shape)
        self.theta = nn.Parameter(init_flat(self.num_items, hidden_dim, latent_dim, self.seed))
        self.register_buffer("steps_done", torch.zeros(1, dtype=torch.int64))
        self.optimizer = pick_optim(config["optim"])(self.parameters(), lr=config["lr"])
        self._fused_adam = self._adam_is_fused()
        self._csr = None              # (device, rowptr, col, users with a train item, nnz_cap) of the dataset's rating matrix
        self._ws = None               # (workspace bytes, layout) on the parameters' device
        self._grad = None             # flat gradient of the last minibatch (foreign optimizers only)
        self._dummy = None            # moment buffers the library is handed when it is only asked for gradients
        self.last_losses = None

    # ------------------------------------------------------------------ the parameters
    def _view(self, name):
        lo, hi, shape = self._slices[name]
        return self.theta.data[lo:hi].view(shape)

    W1 = property(lambda self: self._view("W1"))
    b1 = property(lambda self: self._view("b1"))
    W2 = property(lambda self: self._view("W2"))
    b2 = property(lambda self: self._view("b2"))
    W3 = property(lambda self: self._view("W3"))
    b3 = property(lambda self: self._view("b3"))
    W4 = property(lambda self: self._view("W4"))
    b4 = property(lambda self: self._view("b4"))

    def _device(self):
        dev = self.theta.device
        if dev.type != "cuda":
            raise _lib.HipCallError("Mult-VAE parameters are on the CPU: call .to('cuda') first (no CPU fallback)")
        if not self.theta.data.is_contiguous():
            self.theta.data = self.theta.data.contiguous()
        return dev

    def _ratings(self, dev):
        from .._ratings import rating_csr

        if self._csr is None or self._csr[0] != dev:
            U, I, rowptr, col, _ = rating_csr(self.dataset, dev)
            if (U, I) != (self.num_users, self.num_items):
                raise ValueError(f"Mult-VAE: the dataset's rating matrix is {U} x {I}, its description says {self.num_users} x {self.num_items}")
            if col.numel() == 0:          # an empty matrix still needs an address
                col = torch.zeros(1, dtype=torch.int32, device=dev)
            lens = (rowptr[1:] - rowptr[:-1]).long()
            users = torch.nonzero(lens > 0).view(-1).to(torch.int32).cpu()
            longest = int(lens.max().item()) if U else 0
            nnz_cap = max(1, min(int(rowptr[-1].item()), self.batch_size * longest))
            self._csr = (dev, rowptr.contiguous(), col.contiguous(), users, nnz_cap)
        return self._csr[1:]

    def _moments(self, dev):
        """The flat Adam moments: the entries torch.optim.Adam keeps in optimizer.state, re-homed to the parameters' device when
        they are not there; zeros the library never updates when the optimizer is a foreign one."""
        if not self._fused_adam:
            if self._dummy is None or self._dummy[0].device != dev:
                self._dummy = (torch.zeros_like(self.theta.data), torch.zeros_like(self.theta.data))
            return self._dummy
        st = self._adam_slot(self.theta)
        for k in ("exp_avg", "exp_avg_sq"):
            if st[k].device != dev or not st[k].is_contiguous():
                st[k] = st[k].to(dev).contiguous()
        return st["exp_avg"], st["exp_avg_sq"]

    def _desc(self, dev, training=False, apply_update=True):
        """The descriptor and what keeps its buffers alive."""
        rowptr, col, _, nnz_cap = self._ratings(dev)
        if self._ws is None or self._ws[0].device != dev:
            lay = _lib.MvaeLayout()
            _lib.check(_lib.lib().rk_mvae_workspace(self.num_items, self.hidden, self.latent, self.batch_size, nnz_cap, C.byref(lay)),
                       "rk_mvae_workspace")
            if lay.n_params != self.theta.numel():
                raise _lib.HipCallError(f"rk_mvae_workspace counts {lay.n_params} parameters, the model holds {self.theta.numel()}")
            self._ws = (torch.empty(lay.bytes, dtype=torch.uint8, device=dev), lay)
        ws = self._ws[0]
        m = v = None
        if training:
            m, v = self._moments(dev)
            if not apply_update and (self._grad is None or self._grad.device != dev):
                self._grad = torch.zeros_like(self.theta.data)
        grp = self.optimizer.param_groups[0]
        b1, b2 = grp.get("betas", (0.9, 0.999))
        return _lib.MvaeDesc(
            n_users=self.num_users, n_items=self.num_items, hidden=self.hidden, latent=self.latent, rowptr=rowptr.data_ptr(),
            col=col.data_ptr(), params=self.theta.data.data_ptr(), m=m.data_ptr() if training else None, v=v.data_ptr() if training else None,
            grad=self._grad.data_ptr() if training and not apply_update else None, logits_out=None, dropout=self.dropout,
            anneal_cap=self.anneal_cap, lr=float(grp.get("lr", 1e-3)), beta1=float(b1), beta2=float(b2), adam_eps=float(grp.get("eps", 1e-8)),
            total_anneal_steps=self.total_anneal_steps, seed=self.seed, ws_nnz_cap=nnz_cap, ws_batch=self.batch_size,
            workspace=ws.data_ptr(), workspace_bytes=ws.numel())

    # ------------------------------------------------------------------ training
    def _run_epoch(self, ids, batch, step0, apply_update=True):
        """ceil(n / batch) steps in the library -> double [n_steps, 3] = {loss, mean nll, mean KL} per step, on the device."""
        dev = self._device()
        _lib.require_gpu()
        if apply_update and not self._fused_adam:
            raise _lib.HipCallError("fused update requested with a non-default optimizer (internal error)")
        n = ids.numel()
        if n < 1:
            raise ValueError("Mult-VAE: an epoch without users")
        desc = self._desc(dev, training=True, apply_update=apply_update)
        n_steps = (n + batch - 1) // batch
        losses = torch.empty(3 * n_steps, dtype=torch.float64, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        rc = _lib.lib().rk_mvae_train_epoch(C.byref(desc), _lib.ptr(ids), n, batch, step0, 1 if apply_update else 0, _lib.ptr(losses),
                                            _lib.ptr(status), _lib.stream_ptr(dev))
        bad = device_refusal(rc, "rk_mvae_train_epoch", status)
        if bad:
            raise ValueError(f"Mult-VAE: the epoch's users break rule {bad[0]} ({_lib.RK_MVAE_RULES.get(bad[0], '?')}), first at {bad[1]}")
        if apply_update:
            self.optimizer.state[self.theta]["step"] += n_steps
        return losses.view(n_steps, 3)

    def train_step(self, **config):
        """One epoch over a random order of the users with a train item -> (mean step loss,)."""
        self.train()
        pbar = config.get("progress_bar", None)
        dev = self._device()
        users = self._ratings(dev)[2]
        if users.numel() < 1:
            raise ValueError("Mult-VAE: no user has a train item")
        ids = users[torch.randperm(users.numel())].to(dev).contiguous()       # the global RNG: the workflows re-seed it
        step0 = int(self.steps_done.item())
        if self._fused_adam:
            per_step = self._run_epoch(ids, self.batch_size, step0).cpu()
            self.steps_done += per_step.shape[0]
        else:
            rows = []

            def grad_step(cols):
                part = self._run_epoch(cols[0].contiguous(), max(cols[0].numel(), 1), step0 + len(rows), apply_update=False)
                rows.append(part[0].cpu())
                self.steps_done += 1
                return part[0, 0], {self.theta: self._grad.clone()}

            self._unfused_epoch((ids,), self.batch_size, grad_step)
            per_step = torch.stack(rows)
        mean = per_step.mean(dim=0)
        self.last_losses = {"loss": float(mean[0]), "nll": float(mean[1]), "kl": float(mean[2])}
        if pbar:
            pbar.set_description(f"loss: {self.last_losses['loss']:.4f}")
        return (self.last_losses["loss"],)

    # ------------------------------------------------------------------ scoring
    def forward(self, users, items):
        dev = self._device()
        _lib.require_gpu()
        n = users.numel()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        if n:
            desc = self._desc(dev)
            u, i = (t.to(device=dev, dtype=torch.int32).contiguous() for t in (users, items))
            _lib.check(_lib.lib().rk_mvae_pair_scores(C.byref(desc), _lib.ptr(u), _lib.ptr(i), n, _lib.ptr(out), _lib.stream_ptr(dev)),
                       "rk_mvae_pair_scores")
        return out

    def score_matrix(self, user_ids, out):
        """out[len(user_ids), n_items] <- the inference logit of every item for each user (int32 ids on the device), seen items
        included; the batched evaluation then runs rk_topk_rows on it."""
        dev = self._device()
        _lib.require_gpu()
        desc = self._desc(dev)
        _lib.check(_lib.lib().rk_mvae_scores(C.byref(desc), _lib.ptr(user_ids), user_ids.numel(), _lib.ptr(out), self.num_items,
                                             _lib.stream_ptr(dev)), "rk_mvae_scores")

    def input_describe(self):
        return {
            "train_step": {},
            "forward": {"users": (torch.int64, (VarDim(comment="batch"))), "items": (torch.int64, (VarDim(comment="batch")))},
        }

    def output_describe(self):
        return {
            "train_step": {"loss": (float, [])},
            "forward": {"unnormalized_scores": (torch.float32, [VarDim(comment="batch")])},
        }
