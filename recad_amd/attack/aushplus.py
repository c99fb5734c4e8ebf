"""AushPlus attacker on the device (recad/model/attacker/aushplus.py, registry recad/default.py:187-209).

A GAN whose generator is an autoencoder with a learnable discretisation (DiscretGenerator_AE_1: I -> 125 -> I, tanh, five
rating classes cut by four per-item boundaries, the Heaviside's gradient replaced by tanh's) and whose generator is trained
through the unrolled weighted-MF surrogate of AIA.  csrc/aushplus.hip holds the generator and the discriminator, csrc/aia.hip
the surrogate (this class derives from AIA, as the reference's does, and drives the same entries with variable-length fake
rows); the Adam steps are rk_adam_step over the packed parameter arrays.

Every consumer reads the generator only where its input row is non-zero (value * [x > 0] feeds the discriminator, the
surrogate and generate_fake; the losses select label > 0), so the second layer is a sampled product over a row's non-zeros,
the first layers of G and D are gather-sums over them, and nothing attack_num x I or batch x I is formed.  Gradients of item
rows no entry touches are exactly 0, which Adam leaves where they are, so the optimisers run dense over the arrays.

Behaviour kept from the reference, quirks included:
  * templates are drawn from ALL users (no "at least filler_num ratings" filter, unlike AIA), so a fake row can hold fewer
    than filler_num entries (aushplus.py:23-31);
  * D's optimiser is built from optim_g (with lr_d) (aushplus.py:40); optim_d is never read;
  * the first train_step runs pretrain_epoch_g epochs of pretrain_G and then pretrain_epoch_g (not pretrain_epoch_d) epochs of
    train_D (aushplus.py:163-166);
  * pretrain_G's CrossEntropyLoss takes the five 0/1 products as logits (aushplus.py:144-148);
  * train_D's real side is the first attack_num rows of each dataset batch; a short last batch gives fewer (aushplus.py:113);
  * train_step returns (G_adv_loss, G_rec_loss), both the ATTACK loss of their train_G call: 0.0 for the adversarial phase and
    the last surrogate phase's value (aushplus.py:171-180);
  * an `a` exactly on a boundary gives the all-zero distribution and value 0 (both Heaviside factors are 0 there);
  * generate_fake sets target i to 5 on rows [i * rate, (i + 1) * rate), rate = attack_num // len(targets) (aushplus.py:186-188).
Random calls are the reference's, in its order, on the same generators: np.random.choice of the template users and one
np.random.shuffle per template, the weight initialisation on torch's CPU default generator (init_weights), one
np.random.permutation of the users per pretrain_G / train_D call (dataset.generate_batch), and AIA's per-fit draws.

Deviations: as AIA, a target every real user has rated raises ValueError; the logged MSE and mean score are not computed.
"""
import numpy as np
import torch
from torch import nn

from .. import _lib
from ..utils import VarDim
from . import _common
from .aia import AIA, _BETAS, _EPS

HG, HGR, HD1, HD2 = _lib.RK_AP_HG, _lib.RK_AP_HG_REAL, _lib.RK_AP_HD1, _lib.RK_AP_HD2
EPSILON = 1e-4           # BaseGenerator.epsilon (aushplus.py:236)


def draw_templates(ptr, idx, val, attack_num, filler_num):
    """build_network's draws (aushplus.py:24-30) on a rating CSR: np.random.choice over all users, then per template one
    np.random.shuffle of its nonzero columns, the first filler_num kept.  Returns (users [attack_num], list of the kept
    columns per template in shuffle order; a template with fewer ratings keeps them all)."""
    return _common.draw_templates(ptr, idx, val, attack_num, filler_num, need_filler_num=False)


def init_weights(n_items):
    """The reference's initial parameters, drawn from torch's CPU default generator in its construction order
    (aushplus.py:32-41, 400-475): DiscretGenerator_AE_1's two nn.Linear (default init, consumed), then init_weights' normal_
    per layer (weight std sqrt(2 / (fan_in + fan_out)), bias std 0.001), then the Discriminator's three nn.Linear.
    Returns (generator state, discriminator state) in the reference's parameter names."""
    layers = [nn.Linear(n_items, HGR), nn.Linear(HGR, n_items)]
    for layer in layers:
        fan_out, fan_in = layer.weight.size()
        layer.weight.data.normal_(0.0, np.sqrt(2.0 / (fan_in + fan_out)))
        layer.bias.data.normal_(0.0, 0.001)
    d = [nn.Linear(n_items, HD1), nn.Linear(HD1, HD2), nn.Linear(HD2, 1)]
    gs = {"min_boundary_value": torch.ones(n_items), "interval_lengths": torch.ones(n_items, 3)}
    for k, lin in enumerate(layers):
        gs[f"layers.{k}.weight"], gs[f"layers.{k}.bias"] = lin.weight.detach(), lin.bias.detach()
    ds = {}
    for k, lin in zip((0, 2, 4), d):
        ds[f"main.{k}.weight"], ds[f"main.{k}.bias"] = lin.weight.detach(), lin.bias.detach()
    return gs, ds


def g_offsets(n_items):
    """Offsets of the packed generator (include/recad_hip.h): w1t [I, 128] | b1 [128] | w2 [I, 128] | b2 | min_boundary | lengths."""
    o = {"w1t": 0, "b1": n_items * HG}
    o["w2"] = o["b1"] + HG
    o["b2"] = o["w2"] + n_items * HG
    o["minb"] = o["b2"] + n_items
    o["ilen"] = o["minb"] + n_items
    o["end"] = o["ilen"] + 3 * n_items
    return o


def d_offsets(n_items):
    """Offsets of the packed discriminator: w1t [I, 512] | b1 [512] | W2 [128, 512] | b2 [128] | w3 [128] | b3 [1]."""
    o = {"w1t": 0, "b1": n_items * HD1}
    o["W2"] = o["b1"] + HD1
    o["b2"] = o["W2"] + HD2 * HD1
    o["w3"] = o["b2"] + HD2
    o["b3"] = o["w3"] + HD2
    o["end"] = o["b3"] + 1
    return o


def pack_generator(gs, n_items):
    o = g_offsets(n_items)
    p = torch.zeros(o["end"], dtype=torch.float32)
    p[: o["b1"]].view(n_items, HG)[:, :HGR] = gs["layers.0.weight"].t()
    p[o["b1"]:o["b1"] + HGR] = gs["layers.0.bias"]
    p[o["w2"]:o["b2"]].view(n_items, HG)[:, :HGR] = gs["layers.1.weight"]
    p[o["b2"]:o["minb"]] = gs["layers.1.bias"]
    p[o["minb"]:o["ilen"]] = gs["min_boundary_value"]
    p[o["ilen"]:] = gs["interval_lengths"].reshape(-1)
    return p


def unpack_generator(p, n_items):
    o = g_offsets(n_items)
    p = p.detach().cpu()
    return {"min_boundary_value": p[o["minb"]:o["ilen"]].clone(), "interval_lengths": p[o["ilen"]:].view(n_items, 3).clone(),
            "layers.0.weight": p[: o["b1"]].view(n_items, HG)[:, :HGR].t().contiguous(), "layers.0.bias": p[o["b1"]:o["b1"] + HGR].clone(),
            "layers.1.weight": p[o["w2"]:o["b2"]].view(n_items, HG)[:, :HGR].contiguous(), "layers.1.bias": p[o["b2"]:o["minb"]].clone()}


def pack_discriminator(ds, n_items):
    o = d_offsets(n_items)
    p = torch.empty(o["end"], dtype=torch.float32)
    p[: o["b1"]] = ds["main.0.weight"].t().reshape(-1)
    p[o["b1"]:o["W2"]] = ds["main.0.bias"]
    p[o["W2"]:o["b2"]] = ds["main.2.weight"].reshape(-1)
    p[o["b2"]:o["w3"]] = ds["main.2.bias"]
    p[o["w3"]:o["b3"]] = ds["main.4.weight"].reshape(-1)
    p[o["b3"]:] = ds["main.4.bias"]
    return p


def unpack_discriminator(p, n_items):
    o = d_offsets(n_items)
    p = p.detach().cpu()
    return {"main.0.weight": p[: o["b1"]].view(n_items, HD1).t().contiguous(), "main.0.bias": p[o["b1"]:o["W2"]].clone(),
            "main.2.weight": p[o["W2"]:o["b2"]].view(HD2, HD1).clone(), "main.2.bias": p[o["b2"]:o["w3"]].clone(),
            "main.4.weight": p[o["w3"]:o["b3"]].view(1, HD2).clone(), "main.4.bias": p[o["b3"]:].clone()}


def gather_rows(ptr, idx, val, users):
    """The CSR (rowptr int64, col, val) of rows `users` of a CSR, in that order."""
    users = np.asarray(users, dtype=np.int64)
    lens = ptr[users + 1] - ptr[users]
    rp = np.zeros(len(users) + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lens)
    src = np.repeat(ptr[users] - rp[:-1], lens) + np.arange(rp[-1])
    return rp, idx[src], val[src]


def by_item(cols, rows, n_items):
    """Entries grouped by item, entry order kept inside an item: (tptr [n_items + 1], order) with cols[order] ascending."""
    order = np.argsort(cols, kind="stable")
    tptr = np.zeros(n_items + 1, dtype=np.int64)
    tptr[1:] = np.cumsum(np.bincount(cols, minlength=n_items))
    return tptr, order


class AushPlus(AIA):
    """``model.from_config("attacker", "aushplus", **kw)`` keeps the configuration, ``.I(dataset=explicit)`` draws the templates
    and the weights, ``train_step(target_id_list=...)`` returns (g_adv, g_rec), ``generate_fake(target_id_list=...)`` returns
    an attack_num x n_items float32 array."""

    victim_name = "aushplus"
    scope = "attacker"

    def _build(self, attack_num, filler_num, pretrain_epoch_g, pretrain_epoch_d, epoch_gan_d, epoch_gan_g, epoch_surrogate, lr_g, lr_d,
               optim_g, optim_d, surrogate_model, epoch_s, unroll_steps_s, hidden_dim_s, lr_s, weight_decay_s, batch_size_s,
               weight_pos_s, weight_neg_s, history_bytes, **config):
        self._refuse(config, surrogate_model, weight_neg_s, optim_g, hidden_dim_s, batch_size_s, unroll_steps_s, epoch_s, filler_num,
                     attack_num)
        for k, v in (("pretrain_epoch_g", pretrain_epoch_g), ("epoch_gan_d", epoch_gan_d), ("epoch_gan_g", epoch_gan_g),
                     ("epoch_surrogate", epoch_surrogate)):
            if int(v) < 0:
                raise ValueError(f"AushPlus: {k} {v} must not be negative")
        ds, U, I, ptr, idx, val = _common.open_build(self, config)
        self.dataset, dev = ds, self.device
        self.attack_num, self.filler_num = int(attack_num), int(filler_num)
        self.pretrain_epoch_g, self.epoch_gan_d, self.epoch_gan_g = int(pretrain_epoch_g), int(epoch_gan_d), int(epoch_gan_g)
        self.epoch_surrogate = int(epoch_surrogate)
        self.lr_g, self.lr_d = float(lr_g), float(lr_d)
        self.lr_s, self.wd_s, self.w_pos = float(lr_s), float(weight_decay_s), float(weight_pos_s)
        self.epoch_s, self.unroll, self.dim, self.batch = int(epoch_s), int(unroll_steps_s), int(hidden_dim_s), int(batch_size_s)
        self.history_bytes = int(history_bytes)
        self.batch_size = int(getattr(ds, "config", {}).get("batch_size", 256))
        self.n_users, self.n_items = U, I
        ptr, idx, val = np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(val, np.float32)
        self._host_csr = (ptr, idx, val)
        A = self.attack_num
        # ---- templates (aushplus.py:24-31): variable-length rows, columns ascending
        users, kept = draw_templates(ptr, idx, val, A, self.filler_num)
        self.template_users = users
        trp = np.zeros(A + 1, dtype=np.int64)
        trp[1:] = np.cumsum([len(k) for k in kept])
        tcol = np.concatenate([np.sort(k) for k in kept]) if trp[-1] else np.zeros(0, np.int64)
        tval = np.zeros(int(trp[-1]), dtype=np.float32)
        for r, u in enumerate(users):
            b, e = ptr[u], ptr[u + 1]
            tval[trp[r]:trp[r + 1]] = val[b:e][np.searchsorted(idx[b:e], tcol[trp[r]:trp[r + 1]])]
        self.template_rowptr, self.template_cols, self.template_vals = trp, tcol, tval
        self.n_fake = nf = int(trp[-1])
        trow = np.repeat(np.arange(A), np.diff(trp))
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(dev)   # noqa: E731
        f32 = lambda n: torch.zeros(max(1, int(n)), dtype=torch.float32, device=dev)       # noqa: E731
        self._t_rowptr, self._t_col = i32(trp), i32(tcol if nf else np.zeros(1))
        self._t_x = torch.as_tensor(tval if nf else np.zeros(1, np.float32)).to(dev)
        tptr, order = by_item(tcol, trow, I)
        self._t_tptr, self._t_tent, self._t_trow = i32(tptr), i32(order if nf else np.zeros(1)), i32(trow[order] if nf else np.zeros(1))
        self._t_norm, self._t_h1, self._t_a = f32(A), f32(A * HG), f32(nf)
        self._t_cls = torch.zeros(max(1, nf), dtype=torch.int32, device=dev)
        self._t_scr = {"zbar": f32(nf), "bbar": f32(4 * nf), "eloss": f32(nf), "dpre": f32(A * HG)}
        self._t_din = f32(nf)
        # ---- the surrogate's data: the rating CSR, then the fake rows (AIA's layout with a general rowptr)
        self._surrogate_data(trp[1:], tcol, max(1, nf))
        self.gen = self._x[self.nnz_real:self.nnz_real + nf]       # the generator's value at the template entries
        # ---- the networks (aushplus.py:32-42)
        gs, dstate = init_weights(I)
        self.g_param = pack_generator(gs, I).to(dev)
        self.d_param = pack_discriminator(dstate, I).to(dev)
        self.g_grad, self.g_m, self.g_v = (torch.zeros_like(self.g_param) for _ in range(3))
        self.d_grad, self.d_m, self.d_v = (torch.zeros_like(self.d_param) for _ in range(3))
        self._g_t = self._d_t = 0
        self._d_work = f32((A + min(A, self.batch_size)) * _lib.RK_AP_D_WORK_PER_ROW)
        self.pretrained = False
        self.last_entry = self.last_xbar = self.last_loss = self.last_history = None
        self.last_phase_losses = {}
        self.margin_log = None
        self._forward_templates()

    # ------------------------------------------------------------------ description (aushplus.py:44-48)
    def input_describe(self):
        return {"train_step": {"target_id_list": (list, VarDim())}}

    def output_describe(self):
        return {"train_step": {"g_adv": (float, []), "g_rec": (float, [])}}

    # ------------------------------------------------------------------ accessors
    def generator_state(self):
        """netG.state_dict() of the reference (CPU tensors)."""
        return unpack_generator(self.g_param, self.n_items)

    def discriminator_state(self):
        """netD.state_dict() of the reference (CPU tensors)."""
        return unpack_discriminator(self.d_param, self.n_items)

    def load_generator_state(self, gs):
        self.g_param.copy_(pack_generator({k: torch.as_tensor(v, dtype=torch.float32) for k, v in gs.items()}, self.n_items))

    def load_discriminator_state(self, ds):
        self.d_param.copy_(pack_discriminator({k: torch.as_tensor(v, dtype=torch.float32) for k, v in ds.items()}, self.n_items))

    def last_forward(self):
        """The last template forward at the template entries (row-major, ascending columns): dict of a, cls (-1 = on a
        boundary), value, h1 [attack_num, 125]."""
        nf = self.n_fake
        return {"a": self._t_a[:nf].cpu().numpy(), "cls": self._t_cls[:nf].cpu().numpy(), "value": self.gen.cpu().numpy(),
                "h1": self._t_h1.view(self.attack_num, HG)[:, :HGR].cpu().numpy(), "norm": self._t_norm[: self.attack_num].cpu().numpy()}

    def last_hypergradient(self):
        """dG_loss / d value at the template entries of the last surrogate phase."""
        return self.last_xbar.cpu().numpy()

    def generator_grad(self):
        """The last generator gradient in the reference's parameter names."""
        return unpack_generator(self.g_grad, self.n_items)

    def discriminator_grad(self):
        return unpack_discriminator(self.d_grad, self.n_items)

    def generator_values(self):
        """The generator's value at the template entries (row-major, ascending columns; rows of template_rowptr)."""
        return self.gen.cpu().numpy()

    def _project(self):
        pass        # AIA's rounding of a free parameter has no counterpart: the projection is the generator's own

    # ------------------------------------------------------------------ kernels
    def g_forward(self, rowptr, col, x, n_rows, norm, h1, a, cls, value, span=None):
        P = _lib.ptr
        _lib.check(_lib.lib().rk_ap_g_forward(n_rows, self.n_items, P(rowptr), P(col), P(x), P(self.g_param), P(norm), P(h1), P(a), P(cls),
                                              P(value), self._s()), "rk_ap_g_forward")
        if self.margin_log is not None and span is not None and span[1] > span[0]:
            self.margin_log.append(self._margin(col[span[0]:span[1]], x[span[0]:span[1]], a[span[0]:span[1]]))

    def _margin(self, col, x, a):
        """Diagnostic (margin_log = [] switches it on): min over the consumed entries of min_k |a - b_k|, a device scalar."""
        o, I = g_offsets(self.n_items), self.n_items
        b = [self.g_param[o["minb"]:o["ilen"]]]
        ilen = self.g_param[o["ilen"]:o["end"]].view(I, 3)
        for k in range(3):
            b.append(b[-1] + (torch.relu(ilen[:, k]) + EPSILON))
        d = (a[:, None] - torch.stack(b, 1)[col.long()]).abs().min(1).values
        return torch.where(x > 0, d, torch.full_like(d, float("inf"))).min()

    def run_margin_min(self):
        """The smallest logged margin (one read-back)."""
        return float(torch.stack(self.margin_log).min().cpu())

    def g_backward(self, rowptr, col, x, n_rows, norm, h1, a, mode, dvalue, scale, entry0, n_entries, tptr, tent, trow, scr, loss):
        P = _lib.ptr
        _lib.check(_lib.lib().rk_ap_g_backward(n_rows, self.n_items, P(rowptr), P(col), P(x), P(self.g_param), P(norm), P(h1), P(a), mode,
                                               P(dvalue), scale, entry0, n_entries, P(tptr), P(tent), P(trow), P(scr["zbar"]), P(scr["bbar"]),
                                               P(scr["eloss"]), P(scr["dpre"]), P(self.g_grad), P(loss), self._s()), "rk_ap_g_backward")

    def d_step(self, nA, rowptrA, colA, valA, labelA, nB, labelB, lists, grad, din, loss):
        """D forward / BCE / backward on nA rows of CSR A and the first nB template rows carrying the generator's value."""
        P = _lib.ptr
        n = nA + nB
        if self._d_work.numel() < n * _lib.RK_AP_D_WORK_PER_ROW:
            self._d_work = torch.zeros(n * _lib.RK_AP_D_WORK_PER_ROW, dtype=torch.float32, device=self.device)
        tp, tr, ts = lists if lists is not None else (None, None, None)
        _lib.check(_lib.lib().rk_ap_d_step(self.n_items, nA, P(rowptrA), P(colA), P(valA), labelA, nB, P(self._t_rowptr), P(self._t_col),
                                           P(self._x[self.nnz_real:]), labelB, P(self.d_param), P(self._d_work), P(tp), P(tr), P(ts),
                                           P(self.d_grad) if grad else None, P(din), P(loss), self._s()), "rk_ap_d_step")

    def d_outputs(self, n):
        """D(row) of the last d_step's n rows."""
        o = n * (2 * HD1 + 2 * HD2)
        return self._d_work[o:o + n].cpu().numpy()

    def _adam(self, which):
        if which == "g":
            self._g_t += 1
            p, g, m, v, t, lr = self.g_param, self.g_grad, self.g_m, self.g_v, self._g_t, self.lr_g
        else:
            self._d_t += 1
            p, g, m, v, t, lr = self.d_param, self.d_grad, self.d_m, self.d_v, self._d_t, self.lr_d
        P = _lib.ptr
        _lib.check(_lib.lib().rk_adam_step(p.numel(), P(p), P(g), P(m), P(v), t, lr, _BETAS[0], _BETAS[1], _EPS, self._s()), "rk_adam_step")

    def _forward_templates(self):
        """netG(real_template): a, class and value at the template entries (value lands in the surrogate's data)."""
        if self.n_fake:
            self.g_forward(self._t_rowptr, self._t_col, self._t_x, self.attack_num, self._t_norm, self._t_h1, self._t_a, self._t_cls,
                           self._x[self.nnz_real:], span=(0, self.n_fake))

    def _backward_templates(self, dvalue):
        self.g_backward(self._t_rowptr, self._t_col, self._t_x, self.attack_num, self._t_norm, self._t_h1, self._t_a, 0, dvalue, 0.0, 0,
                        self.n_fake, self._t_tptr, self._t_tent, self._t_trow, self._t_scr, None)

    # ------------------------------------------------------------------ dataset.generate_batch (explicit.py:178-199)
    def epoch_batches(self, take=None, perm=None):
        """One np.random.permutation of the users cut into batches of batch_size, the first `take` rows of each kept (all when
        None): the rows' CSR on the device and, per batch, (first row, row count, first entry, entry count)."""
        if perm is None:
            perm = np.random.permutation(np.arange(self.n_users))
        bs, keep, spans = self.batch_size, [], []
        for b in range((len(perm) + bs - 1) // bs):
            us = perm[b * bs:(b + 1) * bs]
            us = us if take is None else us[:take]
            spans.append((sum(len(k) for k in keep), len(us)))
            keep.append(us)
        users = np.concatenate(keep)
        rp, col, val = gather_rows(*self._host_csr, users)
        dev = self.device
        out = {"users": users, "rowptr_h": rp, "col_h": col, "val_h": val,
               "rowptr": torch.as_tensor(rp.astype(np.int32)).to(dev), "col": torch.as_tensor(col.astype(np.int32)).to(dev),
               "val": torch.as_tensor(val).to(dev),
               "batches": [(r0, n, int(rp[r0]), int(rp[r0 + n] - rp[r0])) for r0, n in spans]}
        return out

    # ------------------------------------------------------------------ aushplus.py:133-158
    def pretrain_G(self, perm=None):
        """One epoch of reconstruction: per dataset batch, G forward on the real rows, the cross-entropy of the five products
        against label - 1 over the batch's non-zeros, one G step.  Returns the mean batch loss (one read-back)."""
        ep = self.epoch_batches(perm=perm)
        dev, I = self.device, self.n_items
        nb = len(ep["batches"])
        losses = torch.zeros(nb, dtype=torch.float32, device=dev)
        max_rows = max(n for _, n, _, _ in ep["batches"])
        E = len(ep["col_h"])
        f32 = lambda n: torch.zeros(max(1, int(n)), dtype=torch.float32, device=dev)       # noqa: E731
        norm, h1, a, value = f32(max_rows), f32(max_rows * HG), f32(E), f32(E)
        cls = torch.zeros(max(1, E), dtype=torch.int32, device=dev)
        scr = {"zbar": f32(E), "bbar": f32(4 * E), "eloss": f32(E), "dpre": f32(max_rows * HG)}
        tptrs, tents, trows, ofs = [], [], [], 0
        for r0, n, k0, ne in ep["batches"]:
            cols = ep["col_h"][k0:k0 + ne]
            rows = np.repeat(np.arange(n), np.diff(ep["rowptr_h"][r0:r0 + n + 1]))
            tptr, order = by_item(cols, rows, I)
            tptrs.append(tptr + ofs)
            tents.append(order + k0)
            trows.append(rows[order])
            ofs += ne
        i32 = lambda a_: torch.as_tensor(np.ascontiguousarray(a_, dtype=np.int32)).to(dev)   # noqa: E731
        tptr_d, tent_d, trow_d = i32(np.stack(tptrs)), i32(np.concatenate(tents + [np.zeros(1)])), i32(np.concatenate(trows + [np.zeros(1)]))
        for bi, (r0, n, k0, ne) in enumerate(ep["batches"]):
            rp = ep["rowptr"][r0:r0 + n + 1]
            self.g_forward(rp, ep["col"], ep["val"], n, norm, h1, a, cls, value, span=(k0, k0 + ne))
            npos = int((ep["val_h"][k0:k0 + ne] > 0).sum())
            self.g_backward(rp, ep["col"], ep["val"], n, norm, h1, a, 1, None, 1.0 / max(1, npos), k0, ne, tptr_d[bi], tent_d, trow_d, scr,
                            losses[bi:])
            self._adam("g")
        self.last_pretrain = {"a": a, "cls": cls, "value": value, "epoch": ep}
        out = losses.cpu().numpy().astype(np.float64)
        self.last_batch_losses = out
        return float(out.mean())

    # ------------------------------------------------------------------ aushplus.py:103-131
    def train_D(self, perm=None):
        """One epoch of the discriminator: G forward on the templates once; per dataset batch BCE(D(first attack_num real rows), 1)
        + BCE(D(fake), 0) and one D step.  Returns the mean batch loss (one read-back)."""
        self._forward_templates()
        A, I, dev = self.attack_num, self.n_items, self.device
        ep = self.epoch_batches(take=A, perm=perm)
        nb = len(ep["batches"])
        losses = torch.zeros(nb, dtype=torch.float32, device=dev)
        trp = self.template_rowptr
        frow = np.repeat(np.arange(A), np.diff(trp))
        tptrs, trows, tsrcs, ofs = [], [], [], 0
        for r0, n, k0, ne in ep["batches"]:
            rows = np.repeat(np.arange(n), np.diff(ep["rowptr_h"][r0:r0 + n + 1]))
            cols = np.concatenate([ep["col_h"][k0:k0 + ne], self.template_cols])
            allrows = np.concatenate([rows, n + frow])
            src = np.concatenate([k0 + np.arange(ne), np.arange(self.n_fake)])
            tptr, order = by_item(cols, allrows, I)
            tptrs.append(tptr + ofs)
            trows.append(allrows[order])
            tsrcs.append(src[order])
            ofs += len(cols)
        i32 = lambda a_: torch.as_tensor(np.ascontiguousarray(a_, dtype=np.int32)).to(dev)   # noqa: E731
        tptr_d, trow_d, tsrc_d = i32(np.stack(tptrs)), i32(np.concatenate(trows + [np.zeros(1)])), i32(np.concatenate(tsrcs + [np.zeros(1)]))
        for bi, (r0, n, k0, ne) in enumerate(ep["batches"]):
            self.d_step(n, ep["rowptr"][r0:r0 + n + 1], ep["col"], ep["val"], 1.0, A, 0.0, (tptr_d[bi], trow_d, tsrc_d), True, None,
                        losses[bi:])
            self._adam("d")
        out = losses.cpu().numpy().astype(np.float64)
        self.last_batch_losses = out
        return float(out.mean())

    # ------------------------------------------------------------------ aushplus.py:50-101
    def train_G_adv(self):
        """train_G(adv=True, attack=False): BCE(D(fake), 1) through D's input into G, one G step.  Returns the loss as a device
        scalar (train_step reads the phase's losses back once)."""
        self._forward_templates()
        loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.d_step(0, None, None, None, 1.0, self.attack_num, 1.0, None, False, self._t_din, loss)
        self._backward_templates(self._t_din)
        self._adam("g")
        return loss

    def train_G_attack(self, target_id_list):
        """train_G(adv=False, attack=True): the value at the template entries is the surrogate's fake data; a fresh fit, the
        attack loss and its gradient at those entries exactly as AIA.train_step, then through the projection and G; one G step.
        Returns the attack loss as a device scalar."""
        self._targets(target_id_list)
        self._forward_templates()
        theta0 = self.init_surrogate()
        idx_list = np.arange(self.R)
        E, K_e = self.epoch_s, self.unroll
        perms, invs = self._perms(idx_list, E)
        dp = torch.as_tensor(perms).to(self.device)
        di = torch.as_tensor(invs).to(self.device)
        state, t = self.run_plain(theta0, dp[: E - K_e], di[: E - K_e])
        self.last_entry = {"state": state, "adam_t": t, "perms": perms[E - K_e:].copy()}
        loss, xbar, _ = self.unrolled(state, t, dp[E - K_e:], di[E - K_e:], target_id_list)
        self.last_xbar = xbar
        if self.n_fake:
            self._backward_templates(xbar)
        else:
            self.g_grad.zero_()
        self._adam("g")
        return loss

    # ------------------------------------------------------------------ aushplus.py:160-180
    def train_step(self, **config):
        target_id_list = config["target_id_list"]
        self._targets(target_id_list)             # refuse bad targets before any draw
        if self.epoch_gan_g == 0 or self.epoch_surrogate == 0:
            raise ValueError("AushPlus.train_step: epoch_gan_g and epoch_surrogate must be positive (the reference's return value is "
                             "unbound otherwise)")
        ph = {}
        if not self.pretrained:
            ph["pretrain_g"] = [self.pretrain_G() for _ in range(self.pretrain_epoch_g)]
            ph["pretrain_d"] = [self.train_D() for _ in range(self.pretrain_epoch_g)]
            self.pretrained = True
        ph["gan_d"] = [self.train_D() for _ in range(self.epoch_gan_d)]
        adv = [self.train_G_adv() for _ in range(self.epoch_gan_g)]
        att = [self.train_G_attack(target_id_list) for _ in range(self.epoch_surrogate)]
        both = torch.cat(adv + att).cpu().numpy().astype(np.float64)      # the GAN and surrogate phases' one read-back
        ph["gan_g"], ph["attack"] = both[: len(adv)].tolist(), both[len(adv):].tolist()
        self.last_phase_losses = ph
        self.last_loss = ph["attack"][-1]
        return (0.0, float(ph["attack"][-1]))

    # ------------------------------------------------------------------ aushplus.py:182-189
    def generate_fake(self, **kwargs):
        """The template forward, each target set to 5 on its attack_num // len(targets) rows."""
        target_id_list = list(kwargs["target_id_list"])
        if not target_id_list:
            raise ValueError("AushPlus: target_id_list is empty")
        if min(target_id_list) < 0 or max(target_id_list) >= self.n_items:
            raise ValueError(f"AushPlus: target ids must lie in [0, {self.n_items})")
        self._forward_templates()
        A = self.attack_num
        out = np.zeros((A, self.n_items), dtype=np.float32)
        rows = np.repeat(np.arange(A), np.diff(self.template_rowptr))
        out[rows, self.template_cols] = self.gen.cpu().numpy()
        rate = int(A / len(target_id_list))
        for i, t in enumerate(target_id_list):
            out[i * rate:(i + 1) * rate, int(t)] = 5
        return out
