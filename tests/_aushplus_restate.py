"""float64 torch restatement of the AushPlus generator (DiscretGenerator_AE_1 with its projection and the tanh surrogate
gradient of the Heaviside, aushplus.py:192-224, 311-378, 400-459) and discriminator (aushplus.py:462-475) on CSR rows, for the
tests of csrc/aushplus.hip.  It is written from the formulas, with autograd doing the backward; nothing here is the
product's code path.  Parameters are dicts in the reference's names."""
import numpy as np
import torch

DT = torch.float64


class HeaviTanh(torch.autograd.Function):
    """forward [x > 0]; backward dy (1 - tanh(x)^2)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return (x > 0).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return dy * (1 - torch.tanh(x) ** 2)


def params64(state, grad=True):
    return {k: torch.as_tensor(np.asarray(v)).to(DT).clone().requires_grad_(grad) for k, v in state.items()}


def rows_of(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return torch.as_tensor(np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)))


def boundaries(gs, eps_dtype=DT):
    """[I, 4]: b0 = min_boundary, b_k = b_{k-1} + relu(len_{k-1}) + 1e-4 (the reference's epsilon is the float32 1e-4)."""
    eps = float(np.float32(1e-4))
    b = [gs["min_boundary_value"]]
    for k in range(1, 4):
        b.append(b[-1] + (torch.relu(gs["interval_lengths"][:, k - 1]) + eps))
    return torch.stack(b, 1)


def g_forward(gs, rowptr, col, x):
    """Returns dict: h1 [rows, 125], a, dist [E, 5], value (unmasked), masked = value [x > 0], margin = min_k |a - b_k|."""
    n = len(rowptr) - 1
    rows = rows_of(rowptr)
    col = torch.as_tensor(np.asarray(col, dtype=np.int64))
    x = torch.as_tensor(np.asarray(x)).to(DT)
    s2 = torch.zeros(n, dtype=DT).index_add(0, rows, x * x)
    h0 = x / torch.sqrt(s2).clamp_min(1e-12)[rows]
    W1, W2 = gs["layers.0.weight"], gs["layers.1.weight"]
    h1 = torch.relu(torch.zeros(n, W1.shape[0], dtype=DT).index_add(0, rows, h0[:, None] * W1.t()[col]) + gs["layers.0.bias"])
    z = (W2[col] * h1[rows]).sum(1) + gs["layers.1.bias"][col]
    a = torch.tanh(z) * 2.5 + 2.5
    d = a[:, None] - boundaries(gs)[col]                     # [E, 4]
    dist = []
    for c in range(5):
        p = torch.ones_like(a)
        for k in range(4):
            p = p * HeaviTanh.apply(np.sign(c - k - 0.5) * d[:, k])
        dist.append(p)
    dist = torch.stack(dist, 1)
    value = dist @ torch.arange(1.0, 6.0, dtype=DT)
    return {"h1": h1, "a": a, "dist": dist, "value": value, "masked": value * (x > 0).to(DT), "margin": d.detach().abs().min(1).values,
            "x": x, "rows": rows, "col": col}


def ce_loss(fw):
    """CrossEntropyLoss of the five products as logits against x - 1 over the entries with x > 0 (aushplus.py:143-148)."""
    sel = fw["x"] > 0
    return torch.nn.functional.cross_entropy(fw["dist"][sel], (fw["x"][sel].long() - 1))


def d_forward(ds, rowptr, col, val):
    """D(rows) [n]: val may be a tensor in the graph (the generator's masked value) or an array (ratings)."""
    n = len(rowptr) - 1
    rows = rows_of(rowptr)
    col = torch.as_tensor(np.asarray(col, dtype=np.int64))
    v = val if torch.is_tensor(val) else torch.as_tensor(np.asarray(val)).to(DT)
    W1 = ds["main.0.weight"]
    h1 = torch.relu(torch.zeros(n, W1.shape[0], dtype=DT).index_add(0, rows, v[:, None] * W1.t()[col]) + ds["main.0.bias"])
    h2 = torch.relu(h1 @ ds["main.2.weight"].t() + ds["main.2.bias"])
    return torch.sigmoid(h2 @ ds["main.4.weight"].t() + ds["main.4.bias"])[:, 0]


def bce(p, label):
    return torch.nn.functional.binary_cross_entropy(p, torch.full_like(p, label))


def adam_first_step(p, g, lr):
    """torch.optim.Adam's first step from m = v = 0 (float64)."""
    m, v = 0.1 * g, 0.001 * g * g
    return p - lr / 0.1 * m / (np.sqrt(v) / np.sqrt(0.001) + 1e-8)
