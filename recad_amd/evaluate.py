"""Batched full-catalog scoring + top-K + HR@K on device.

Replaces the per-user Python loop + pandas sort of Normal.user_item_model_generate
(recad/workflow/normal.py:57-93) with rk_score_topk: propagate ONCE, then for blocks of
users one fp32-MFMA GEMM and one selection kernel.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .utils import get_logger


def score_plan(nb, n_items, dim, K, n_targets, request=None):
    """rk_score_topk_plan: the library's path choice for this request, or the requested one.  request: None / dict with any of
    path ("gemm" | "panel" | "auto"), panel_rows (16 | 32), panel_ntw (8 | 15), panel_safe (bool) -- what the tests and the
    probes force; the product passes None."""
    req = _lib.ScorePlan()
    if request:
        req.path = {"auto": _lib.RK_SCORE_AUTO, "gemm": _lib.RK_SCORE_GEMM, "panel": _lib.RK_SCORE_PANEL}[request.get("path", "auto")]
        req.panel_rows, req.panel_ntw = int(request.get("panel_rows", 0)), int(request.get("panel_ntw", 0))
        req.panel_safe = 1 if request.get("panel_safe") else 0
    out = _lib.ScorePlan()
    _lib.check(_lib.lib().rk_score_topk_plan(int(nb), int(n_items), int(dim), int(K), int(n_targets), C.byref(req) if request else None,
                                             C.byref(out)), "rk_score_topk_plan")
    return out


def tables_finite(*tabs):
    """True when every scoring table (tensor, float or None) is finite.  One reduction per table and ONE read-back: the panel path
    of rk_score_topk requires finite tables (include/recad_hip.h), so a plan that took it is checked once per evaluation and a
    table with a NaN or an infinity goes through RK_SCORE_GEMM, whose selection ranks keys."""
    ok = None
    for t in tabs:
        if t is None:
            continue
        if not torch.is_tensor(t):
            if not np.isfinite(float(t)):
                return False
            continue
        f = torch.isfinite(t).all()
        ok = f if ok is None else ok & f
    return True if ok is None else bool(ok)


# what full_catalog_topk asks the library for when its caller does not say: None = the library's choice.  The GPU tests and the
# probes set it (tests/conftest-style fixtures) -- the library itself reads no environment variable for this any more.
SCORE_REQUEST = None


def full_catalog_topk(victim, user_ids, seen_ptr, seen_idx, targets, K=100, chunk=4096, to_host=True, request=None, extra_scratch_floats=0):
    """For every user in user_ids (int array): top-K unseen items and the score/rank of each target.

    seen_ptr/seen_idx: CSR (indexed by user id) of the items to exclude (the train items), item ids ASCENDING
    within a user (dataset.train_csr_sorted()): the fused sweep walks each list with a cursor.  Host arrays are
    checked and sorted here when needed; device tensors are taken as sorted.
    Returns dict of arrays top_ids[n,K], top_scores[n,K], target_score[n,T], target_rank[n,T]: host numpy
    arrays, or (to_host=False) device tensors left in HBM, no synchronisation -- except when the plan takes the panel path, which
    requires finite tables (include/recad_hip.h): the tables are then checked first, one reduction and ONE read-back per call
    (tables_finite; its cost next to a panel sweep has not been measured), and tables that are not finite go through the GEMM path.
    """
    _lib.require_gpu()
    if request is None:
        request = SCORE_REQUEST
    tabs = victim.scoring_tables() if hasattr(victim, "scoring_tables") else None
    dot = tabs is not None
    if dot:
        utab, itab, ubias, ibias, mean = tabs
        dev = itab.device
        utab, itab = utab.contiguous(), itab.contiguous()
        if ubias is not None:
            ubias, ibias = ubias.contiguous().view(-1), ibias.contiguous().view(-1)
        n_items, d = itab.shape
    else:  # score_matrix(user_ids, out) victims (NCF): scores are not a dot product
        dev = next(victim.parameters()).device
        n_items = victim.num_items
    as_dev = lambda a: (a.to(device=dev, dtype=torch.int32) if torch.is_tensor(a)
                        else torch.as_tensor(np.asarray(a), dtype=torch.int32, device=dev)).contiguous()
    if not torch.is_tensor(seen_idx) and len(seen_idx) > 1:
        sp, si = np.asarray(seen_ptr).astype(np.int64), np.asarray(seen_idx)
        row = np.repeat(np.arange(len(sp) - 1, dtype=np.int64), np.diff(sp))
        key = row * (int(si.max()) + 1) + si
        if not bool(np.all(key[1:] >= key[:-1])):
            seen_idx = si[np.argsort(key, kind="stable")]
    user_ids_t, seen_ptr_t, seen_idx_t = as_dev(user_ids), as_dev(seen_ptr), as_dev(seen_idx)
    if seen_idx_t.numel() == 0:
        seen_idx_t = torch.zeros(1, dtype=torch.int32, device=dev)
    targets_t = as_dev(targets)
    n, T = user_ids_t.numel(), targets_t.numel()
    top_ids = torch.empty(n, K, dtype=torch.int32, device=dev)
    top_scores = torch.empty(n, K, dtype=torch.float32, device=dev)
    tscore = torch.empty(n, max(T, 1), dtype=torch.float32, device=dev)
    trank = torch.empty(n, max(T, 1), dtype=torch.int32, device=dev)
    chunk = max(1, min(chunk, n))
    plan = None
    if dot:
        # the scoring path is an argument of the call: a plan for the whole user list first -- if the library (or the request)
        # takes the panel form, its scratch does not grow with the block, so everything goes in ONE call; the GEMM + selection
        # path works through blocks of `chunk` users (its scratch is the block's score matrix)
        plan = score_plan(n, n_items, d, K, T, request)
        if plan.path == _lib.RK_SCORE_PANEL and not tables_finite(utab, itab, ubias, ibias, mean):
            request = {"path": "gemm"}      # the panel path requires finite tables (recad_hip.h): a diverged victim is ranked by keys
            plan = score_plan(n, n_items, d, K, T, request)
        if plan.path != _lib.RK_SCORE_PANEL:
            plan = score_plan(chunk, n_items, d, K, T, request)
        else:
            chunk = n
        scratch = torch.empty(int(plan.scratch_floats) + extra_scratch_floats, dtype=torch.float32, device=dev)
    else:
        scratch = torch.empty(chunk * n_items, dtype=torch.float32, device=dev)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        ids = user_ids_t[s:e]
        if not dot:
            victim.score_matrix(ids, scratch[: (e - s) * n_items])
            _lib.check(_lib.lib().rk_topk_rows(
                _lib.ptr(scratch), e - s, n_items, _lib.ptr(ids), _lib.ptr(seen_ptr_t), _lib.ptr(seen_idx_t), K,
                _lib.ptr(top_ids[s:e]), _lib.ptr(top_scores[s:e]), _lib.ptr(targets_t), T, _lib.ptr(tscore[s:e]),
                _lib.ptr(trank[s:e]), _lib.stream_ptr()), "rk_topk_rows")
            continue
        _lib.check(_lib.lib().rk_score_topk(
            d, _lib.ptr(utab), e - s, _lib.ptr(ids), _lib.ptr(itab), n_items, _lib.ptr(ubias), _lib.ptr(ibias),
            float(mean), _lib.ptr(seen_ptr_t), _lib.ptr(seen_idx_t), K, _lib.ptr(top_ids[s:e]), _lib.ptr(top_scores[s:e]),
            _lib.ptr(targets_t), T, _lib.ptr(tscore[s:e]), _lib.ptr(trank[s:e]), C.byref(plan), _lib.ptr(scratch), _lib.stream_ptr()),
            "rk_score_topk")
    if not to_host:
        return {"top_ids": top_ids, "top_scores": top_scores, "target_score": tscore[:, :T], "target_rank": trank[:, :T]}
    return {
        "top_ids": top_ids.cpu().numpy(), "top_scores": top_scores.cpu().numpy(),
        "target_score": tscore[:, :T].cpu().numpy(), "target_rank": trank[:, :T].cpu().numpy(),
    }


class EvalSession:
    """A full evaluation of ONE victim on a FIXED user list, set up once and run many times (normal.py:57-93,111-160: propagate,
    score every unseen item, top-K, target score / rank, HR@k numerators): every buffer, the scoring plan and the argument
    marshalling are made in __init__, run() only launches -- and, from its second call on (graph=True), replays ONE hipGraph
    holding the victim's propagation, the GEMM + selection launches of every user block and the HR@k reduction, so an
    evaluation costs one enqueue instead of a Python loop (the perturb-retrain loops that re-score a victim after every
    epoch, bench.py's scorings / s).  Results are device tensors owned by the session, overwritten by the next run().

    A plan that takes the panel path requires finite tables (include/recad_hip.h), so EVERY run() of such a plan first asks
    _panel_ok(), in front of the launch or the replay and outside the captured region: one reduction per table and one read-back
    (a host synchronisation whose cost next to a panel sweep has not been measured).  Tables are trained in place between runs --
    also by the library's own Adam, through raw pointers that move no version counter -- so nothing is cached.  Victims with
    static tables (MF) have the tables themselves checked; victims whose tables come out of a propagation (LightGCN) have the
    propagation's INPUTS checked, their parameters.  That rests on an assumption: the propagation is a normalised average
    (weights in (0, 1], a mean over the layers), which keeps finite inputs finite unless they lie within a factor of the largest
    degree of FLT_MAX; such parameters are not caught.  Not finite: the same evaluation through the GEMM path, with a graph of
    its own.

    The graph holds the victim's table / workspace pointers: it is re-captured when the victim's native handle changes
    (new graph, new dimension), and never used for victims without scoring_tables() (NCF: score_matrix) or with a
    host-synchronising propagation (fuse_layers)."""

    def __init__(self, victim, user_ids, seen_ptr, seen_idx, targets, K=100, topks=(10, 20, 50, 100), chunk=None, request=None, graph=True,
                 quality=None):
        """quality: None, or the (gt_ptr, gt_idx) CSR of a held-out split (rank_metrics): run() then also launches
        rk_rank_metrics over top_ids for `topks` -- inside the captured graph -- and returns its sums as quality_out."""
        _lib.require_gpu()
        if not hasattr(victim, "scoring_tables"):
            raise TypeError("EvalSession needs a victim with scoring_tables() (dot-product scoring); use full_catalog_topk")
        self.victim, self.K, self.topks = victim, int(K), tuple(int(k) for k in topks)
        self.request = SCORE_REQUEST if request is None else request
        tabs = victim.scoring_tables()
        if tabs is None:
            raise TypeError("EvalSession: the victim scores through score_matrix() right now (logit dropout active); use full_catalog_topk")
        # victims whose tables are plain parameter views (MF: scoring_tables_static) are asked once -- their scoring_tables() reads
        # a scalar back, which a stream capture does not allow; LightGCN's launches the propagation and is called per run
        self._static = bool(getattr(victim, "scoring_tables_static", False))
        self._static_tabs = tabs if self._static else None
        self._static_key = self._tables_key()
        utab, itab = tabs[0], tabs[1]
        dev = itab.device
        self.dev = dev
        as_dev = lambda a: (a.to(device=dev, dtype=torch.int32) if torch.is_tensor(a)
                            else torch.as_tensor(np.asarray(a), dtype=torch.int32, device=dev)).contiguous()
        self.users, self.seen_ptr, self.seen_idx, self.targets = as_dev(user_ids), as_dev(seen_ptr), as_dev(seen_idx), as_dev(targets)
        if self.seen_idx.numel() == 0:
            self.seen_idx = torch.zeros(1, dtype=torch.int32, device=dev)
        n, T = self.users.numel(), self.targets.numel()
        self.n, self.T = n, T
        n_items, d = itab.shape
        if chunk is None:
            chunk = max(256, min(8192, (1 << 31) // max(n_items, 1)))
        chunk = max(1, min(int(chunk), max(n, 1)))
        self._gemm_chunk, self._gemm = chunk, None      # (the fallback of a panel plan whose tables are not finite: made when first needed)
        plan = score_plan(max(n, 1), n_items, d, self.K, T, self.request)
        if plan.path != _lib.RK_SCORE_PANEL:
            plan = score_plan(chunk, n_items, d, self.K, T, self.request)
        else:
            chunk = max(n, 1)
        self.plan, self.chunk = plan, chunk
        self.scratch = torch.empty(int(plan.scratch_floats), dtype=torch.float32, device=dev)
        self.top_ids = torch.empty(n, self.K, dtype=torch.int32, device=dev)
        self.top_scores = torch.empty(n, self.K, dtype=torch.float32, device=dev)
        self.tscore = torch.empty(n, max(T, 1), dtype=torch.float32, device=dev)
        self.trank = torch.empty(n, max(T, 1), dtype=torch.int32, device=dev)
        self.ks = torch.as_tensor(list(self.topks), dtype=torch.int32, device=dev)
        self.counts = torch.zeros(max(T, 1), len(self.topks), dtype=torch.int32, device=dev)
        self.quality = None
        if quality is not None:
            disc, qks = _rank_tables(dev, self.K, self.topks)
            gt_ptr, gt_idx = _heldout_csr_device(quality[0], quality[1], dev)
            nk = len(self.topks)
            self.quality = {"gt_ptr": gt_ptr, "gt_idx": gt_idx, "discount": disc, "ks": qks,
                            "hits": torch.empty(n, nk, dtype=torch.int32, device=dev), "dcg": torch.empty(n, nk, dtype=torch.float64, device=dev),
                            "first": torch.empty(n, dtype=torch.int32, device=dev), "out": torch.empty(1 + 5 * nk, dtype=torch.float64, device=dev)}
        self.want_graph = bool(graph) and not getattr(victim, "fuse_layers", False)
        self._graph, self._graph_key, self._runs = None, None, 0

    def _tables_key(self):
        """Static victims (MF): what the cached tables -- and a captured graph's pointers and baked `mean` -- depend on
        (victim.scoring_tables_key(): storages, shapes, `mean`'s version, dropout state; no device read)."""
        if not self._static:
            return None
        fn = getattr(self.victim, "scoring_tables_key", None)
        return fn() if fn is not None else tuple((t.data_ptr(), tuple(t.shape)) for t in self._static_tabs[:4] if t is not None)

    def _refresh_static(self):
        """Called by run() in front of every launch / replay: re-query a static victim's tables when their key moved."""
        if not self._static:
            return
        key = self._tables_key()
        if key != self._static_key:
            tabs = self.victim.scoring_tables()
            if tabs is None:
                raise RuntimeError("EvalSession: the victim scores through score_matrix() now (logit dropout active); use full_catalog_topk")
            if tuple(tabs[1].shape) != (self.plan.n_items, self.plan.dim):
                raise RuntimeError("EvalSession: the victim's item table changed shape; build a new session")
            self._static_tabs, self._static_key = tabs, key
            self._graph, self._graph_key = None, None     # the captured pointers / mean are stale: direct launches, re-capture

    def _panel_ok(self):
        """Panel plans only: are the tables the plan is about to score finite?  (class docstring)"""
        if self._static:      # (on every run: in-place training moves no key)
            return tables_finite(*self._static_tabs)
        params = getattr(self.victim, "parameters", None)
        if params is None:        # no parameters to ask: the tables themselves (LightGCN-like victims: one more propagation)
            return tables_finite(*self.victim.scoring_tables())
        return tables_finite(*[p.detach() for p in params()])

    def _launch(self, use_gemm=False):
        v, L, plan = self.victim, _lib.lib(), self.plan
        utab, itab, ubias, ibias, mean = self._static_tabs if self._static_tabs is not None else v.scoring_tables()   # (LightGCN: the propagation's launches)
        utab, itab = utab.contiguous(), itab.contiguous()
        if ubias is not None:
            ubias, ibias = ubias.contiguous().view(-1), ibias.contiguous().view(-1)
        n_items, d = itab.shape
        chunk, scratch = self.chunk, self.scratch
        if use_gemm:
            if self._gemm is None:
                gplan = score_plan(self._gemm_chunk, n_items, d, self.K, self.T, {"path": "gemm"})
                self._gemm = (gplan, torch.empty(int(gplan.scratch_floats), dtype=torch.float32, device=self.dev))
            (plan, scratch), chunk = self._gemm, self._gemm_chunk
        st = _lib.stream_ptr()
        for s in range(0, self.n, chunk):
            e = min(self.n, s + chunk)
            _lib.check(L.rk_score_topk(
                d, _lib.ptr(utab), e - s, _lib.ptr(self.users[s:e]), _lib.ptr(itab), n_items, _lib.ptr(ubias), _lib.ptr(ibias), float(mean),
                _lib.ptr(self.seen_ptr), _lib.ptr(self.seen_idx), self.K, _lib.ptr(self.top_ids[s:e]), _lib.ptr(self.top_scores[s:e]),
                _lib.ptr(self.targets), self.T, _lib.ptr(self.tscore[s:e]), _lib.ptr(self.trank[s:e]), C.byref(plan), _lib.ptr(scratch), st),
                "rk_score_topk")
        if self.T and self.n:
            _lib.check(L.rk_hit_counts(_lib.ptr(self.trank), self.n, self.T, _lib.ptr(self.ks), len(self.topks), _lib.ptr(self.counts), st), "rk_hit_counts")
        if self.quality is not None:
            q = self.quality
            _lib.check(L.rk_rank_metrics(_lib.ptr(self.top_ids), self.n, self.K, _lib.ptr(self.users), _lib.ptr(q["gt_ptr"]), _lib.ptr(q["gt_idx"]),
                                         _lib.ptr(q["ks"]), len(self.topks), _lib.ptr(q["discount"]), _lib.ptr(q["hits"]), _lib.ptr(q["dcg"]),
                                         _lib.ptr(q["first"]), _lib.ptr(q["out"]), st), "rk_rank_metrics")

    def run(self):
        """-> dict of device tensors (top_ids [n, K], top_scores, target_score [n, T], target_rank, hit_counts [T, len(topks)], and
        with quality= the sums quality_out [1 + 5 len(topks)] of rk_rank_metrics); no synchronisation, but for the table check of a plan
        that takes the panel path (class docstring)."""
        self._runs += 1
        self._refresh_static()
        use_gemm = self.plan.path == _lib.RK_SCORE_PANEL and not self._panel_ok()
        key = (getattr(self.victim, "_handle_key", None), self._static_key, use_gemm)
        if self.want_graph and self._graph is not None and self._graph_key == key:
            self._graph.replay()
        else:
            self._launch(use_gemm)
            if self.want_graph and self._runs >= 2 and (self._graph is None or self._graph_key != key):
                # capture on the SECOND run (a single evaluation never pays for a capture; handles, plans and lazily built
                # schedules exist by now); a failed capture keeps the eager path
                try:
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self._launch(use_gemm)
                    self._graph, self._graph_key = g, (getattr(self.victim, "_handle_key", None), self._static_key, use_gemm)
                    self._graph.replay()     # (the capture itself ran nothing: results must come from an execution)
                except Exception as exc:    # noqa: BLE001
                    import warnings
                    warnings.warn(f"EvalSession: hipGraph capture unavailable ({type(exc).__name__}: {exc}); evaluating with direct launches")
                    self.want_graph, self._graph = False, None
                    torch.cuda.synchronize()
        res = {"top_ids": self.top_ids, "top_scores": self.top_scores, "target_score": self.tscore[:, :self.T],
               "target_rank": self.trank[:, :self.T], "hit_counts": self.counts[: max(self.T, 0)]}
        if self.quality is not None:
            res["quality_out"] = self.quality["out"]
        return res


_KS_CACHE = {}


def hit_counts(target_rank, topks):
    """HR@k numerators on the device: int32 tensor [n_targets, len(topks)] with the number of users whose
    target ranks below k (normal.py:86-92); divide by the number of users for HR@k.  No synchronisation."""
    n, T = target_rank.shape
    key = (target_rank.device, tuple(int(k) for k in topks))
    ks = _KS_CACHE.get(key)
    if ks is None:  # a host->device copy per call would stall the stream
        ks = _KS_CACHE[key] = torch.as_tensor(list(key[1]), dtype=torch.int32, device=target_rank.device)
    counts = torch.empty(T, len(ks), dtype=torch.int32, device=target_rank.device)
    _lib.check(_lib.lib().rk_hit_counts(_lib.ptr(target_rank.contiguous()), n, T, _lib.ptr(ks), len(ks), _lib.ptr(counts),
                                        _lib.stream_ptr()), "rk_hit_counts")
    return counts


RANK_METRICS = ("Recall", "Precision", "NDCG", "HitRate", "MRR")   # the order of rk_rank_metrics' sums per cut-off
_RANK_CACHE = {}


def _rank_tables(device, K, topks):
    """(discount double[K] = 1 / log2(j + 2), ks int32[len(topks)]) on the device, made once per (device, K, topks)."""
    key = (torch.device(device), int(K), tuple(int(k) for k in topks))
    tabs = _RANK_CACHE.get(key)
    if tabs is None:
        K, ks = key[1], key[2]
        if not 1 <= len(ks) <= _lib.RK_RANK_MAX_NK:
            raise ValueError(f"rank_metrics: between 1 and {_lib.RK_RANK_MAX_NK} cut-offs, got {len(ks)}")
        if any(not 1 <= k <= K for k in ks):   # (the kernel cannot refuse what lives in device memory: it clamps)
            raise ValueError(f"rank_metrics: every cut-off must be in [1, K = {K}], got {list(ks)}")
        disc = 1.0 / np.log2(np.arange(K, dtype=np.float64) + 2.0)
        tabs = _RANK_CACHE[key] = (torch.as_tensor(disc, dtype=torch.float64, device=key[0]), torch.as_tensor(list(ks), dtype=torch.int32, device=key[0]))
    return tabs


def _heldout_csr_device(gt_ptr, gt_idx, device):
    """The held-out CSR as int32 device tensors: host arrays are made sorted and unique per row, device tensors are taken as such."""
    if not (torch.is_tensor(gt_ptr) and torch.is_tensor(gt_idx)):
        from .dataset import _sorted_unique_rows
        as_np = lambda a: a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        gt_ptr, gt_idx = _sorted_unique_rows(as_np(gt_ptr).astype(np.int64), as_np(gt_idx))
        gt_ptr, gt_idx = torch.as_tensor(gt_ptr), torch.as_tensor(gt_idx)
    ptr, idx = (a.to(device=device, dtype=torch.int32).contiguous() for a in (gt_ptr, gt_idx))
    if idx.numel() == 0:
        idx = torch.zeros(1, dtype=torch.int32, device=device)
    return ptr, idx


def quality_dict(out, topks):
    """rk_rank_metrics' host-side `out` as {Recall@k, Precision@k, NDCG@k, HitRate@k, MRR@k for every k, n_quality_users}: the sums
    divided by the number of counted users (none: NaN, like Normal._evaluate_on_device)."""
    out = np.asarray(out, dtype=np.float64)
    cnt = float(out[0])
    res = OrderedDict()
    for q, k in enumerate(topks):
        for j, name in enumerate(RANK_METRICS):
            res[f"{name}@{int(k)}"] = float(out[1 + 5 * q + j] / cnt) if cnt > 0 else float("nan")
    res["n_quality_users"] = int(cnt)
    return res


def rank_metrics(top_ids, user_ids, gt_ptr, gt_idx, topks, to_host=True):
    """Held-out ranking quality of the lists full_catalog_topk left on the device (rk_rank_metrics): row b of top_ids [n, K] is the
    list of user user_ids[b]; gt_ptr / gt_idx is the CSR of a held-out split indexed by user id (host arrays are sorted and
    deduplicated here; device tensors are taken as sorted).  to_host=True: an OrderedDict (quality_dict) from ONE read-back of the
    sums; to_host=False: the device tensors (hits [n, nk], dcg [n, nk], first [n], out [1 + 5 nk]), no synchronisation."""
    _lib.require_gpu()
    if not (torch.is_tensor(top_ids) and top_ids.is_cuda and top_ids.dtype == torch.int32 and top_ids.dim() == 2):
        raise TypeError("rank_metrics: top_ids must be the int32 device tensor [n, K] that full_catalog_topk(to_host=False) returns, got "
                        + (f"{top_ids.dtype} {tuple(top_ids.shape)} on {top_ids.device}" if torch.is_tensor(top_ids) else type(top_ids).__name__))
    top_ids = top_ids.contiguous()   # (held by this name until the call below has been enqueued)
    n, K = top_ids.shape
    dev = top_ids.device
    topks = tuple(int(k) for k in topks)
    disc, ks = _rank_tables(dev, K, topks)
    ptr, idx = _heldout_csr_device(gt_ptr, gt_idx, dev)
    users = (user_ids.to(device=dev, dtype=torch.int32) if torch.is_tensor(user_ids)
             else torch.as_tensor(np.asarray(user_ids), dtype=torch.int32, device=dev)).contiguous()
    if users.numel() != n:
        raise ValueError(f"rank_metrics: {n} lists for {users.numel()} users")
    nk = len(topks)
    hits = torch.empty(n, nk, dtype=torch.int32, device=dev)
    dcg = torch.empty(n, nk, dtype=torch.float64, device=dev)
    first = torch.empty(n, dtype=torch.int32, device=dev)
    out = torch.empty(1 + 5 * nk, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().rk_rank_metrics(_lib.ptr(top_ids), n, K, _lib.ptr(users), _lib.ptr(ptr), _lib.ptr(idx), _lib.ptr(ks), nk,
                                          _lib.ptr(disc), _lib.ptr(hits), _lib.ptr(dcg), _lib.ptr(first), _lib.ptr(out), _lib.stream_ptr()),
               "rk_rank_metrics")
    if not to_host:
        return hits, dcg, first, out
    return quality_dict(out.cpu().numpy(), topks)


def heldout_quality(victim, dataset, split="test", topks=(10, 20, 50, 100), users=None, request=None):
    """How good is this victim: Recall / Precision / NDCG / HitRate / MRR @k of its full-catalogue lists (train items excluded)
    against the `split` ("valid" | "test") items of every user who has some -- intersected with `users` when given.  Scoring is
    full_catalog_topk's (all three victims), the metrics rk_rank_metrics'; one read-back."""
    if split not in ("valid", "test"):
        raise ValueError(f"heldout_quality: split must be 'valid' or 'test', got {split!r}")
    if not (hasattr(victim, "scoring_tables") or hasattr(victim, "score_matrix")):
        raise TypeError(f"heldout_quality needs a victim with scoring_tables() or score_matrix(); {type(victim).__name__} has neither")
    if dataset.config.get("graph_source") == "reference":
        get_logger(__name__).warning(f"heldout_quality: graph_source='reference' trains the victim on the test edges; '{split}' quality is not held out")
    gt_ptr, gt_idx = dataset.heldout_csr(split)
    ids = np.nonzero(np.diff(gt_ptr) > 0)[0]
    if users is not None:
        ids = np.intersect1d(ids, (users.cpu().numpy() if torch.is_tensor(users) else np.asarray(users)).astype(np.int64))
    ids = ids.astype(np.int32)
    topks = tuple(int(k) for k in topks)
    if len(ids) == 0:
        return quality_dict(np.zeros(1 + 5 * len(topks)), topks)
    seen_ptr, seen_idx = dataset.train_csr_sorted()
    res = full_catalog_topk(victim, ids, seen_ptr, seen_idx, np.zeros(0, dtype=np.int32), K=max(topks), to_host=False, request=request)
    top_ids = res["top_ids"]
    return rank_metrics(top_ids, ids, *dataset.heldout_csr(split, device=top_ids.device), topks)   # (the device copy is made once per split)


def eligible_users_device(seen_ptr, seen_idx, targets, device):
    """eligible_users() on the device (rk_eligible_users): -> (user_ids int32 device tensor [n], the seen CSR and the
    targets as int32 device tensors).  One scalar read-back (the count sizes every later buffer)."""
    _lib.require_gpu()
    as_dev = lambda a: (a.to(device=device, dtype=torch.int32) if torch.is_tensor(a)
                        else torch.as_tensor(np.asarray(a), dtype=torch.int32, device=device)).contiguous()
    ptr, idx, tg = as_dev(seen_ptr), as_dev(seen_idx), as_dev(targets)
    if idx.numel() == 0:
        idx = torch.zeros(1, dtype=torch.int32, device=device)
    U = ptr.numel() - 1
    flags = torch.empty(max(U, 1), dtype=torch.int32, device=device)
    ids = torch.empty(max(U, 1), dtype=torch.int32, device=device)
    count = torch.zeros(1, dtype=torch.int32, device=device)
    _lib.check(_lib.lib().rk_eligible_users(U, _lib.ptr(ptr), _lib.ptr(idx), _lib.ptr(tg), tg.numel(), _lib.ptr(flags), _lib.ptr(ids),
                                            _lib.ptr(count), _lib.stream_ptr()), "rk_eligible_users")
    return ids[: int(count.item())], ptr, idx, tg


def pred_shift(score_before, score_after):
    """mean(score_after - score_before) over all (user, target) rows (normal.py:147-149) as a device double[2]
    tensor {mean, sum}; no synchronisation."""
    a, b = score_before.contiguous().view(-1), score_after.contiguous().view(-1)
    out = torch.empty(2, dtype=torch.float64, device=a.device)
    _lib.check(_lib.lib().rk_pred_shift(_lib.ptr(a), _lib.ptr(b), a.numel(), _lib.ptr(out), _lib.stream_ptr()), "rk_pred_shift")
    return out


def eligible_users(train_ptr, train_idx, targets):
    """Users the reference evaluates (normal.py:133-143): every user with a train list that
    contains none of the targets."""
    train_ptr = np.asarray(train_ptr)
    train_idx = np.asarray(train_idx)
    U = len(train_ptr) - 1
    deg = np.diff(train_ptr)
    has_target = np.zeros(U, dtype=bool)
    rows = np.repeat(np.arange(U), deg)
    hit = np.isin(train_idx, np.asarray(targets))
    has_target[rows[hit]] = True
    return np.nonzero((deg > 0) & ~has_target)[0].astype(np.int32)


def hr_rows(user_ids, res, topks):
    """[user, score(target), hit@k...] rows like normal.py:89-92 (one target per row)."""
    rows = []
    T = res["target_score"].shape[1]
    for t in range(T):
        hits = [(res["target_rank"][:, t] < k).astype(np.float64) for k in topks]
        rows.append(np.stack([np.asarray(user_ids, dtype=np.float64), res["target_score"][:, t].astype(np.float64)] + hits, 1))
    return np.concatenate(rows, 0) if rows else np.zeros((0, 2 + len(topks)))


def detection_quality(flagged, n_real_users, n_total_users):
    """How many of the users a defender flagged were injected: the fake users are the ids n_real_users .. n_total_users - 1
    (inject_data appends them).  Plain host arithmetic over the DISTINCT flagged ids; an id outside [0, n_total_users) is
    ignored (it names nobody, so it is neither a hit nor a false alarm).  precision = 0 when nothing is flagged, recall = 0
    when nothing is fake, f1 = 0 when both are 0."""
    n_real, n_total = int(n_real_users), int(n_total_users)
    if not 0 <= n_real <= n_total:
        raise ValueError(f"detection_quality: n_real_users = {n_real} outside 0..n_total_users = {n_total}")
    ids = {int(u) for u in flagged if 0 <= int(u) < n_total}
    tp, n_fake = sum(1 for u in ids if u >= n_real), n_total - n_real
    precision = tp / len(ids) if ids else 0.0
    recall = tp / n_fake if n_fake else 0.0
    f1 = 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    return {"precision": precision, "recall": recall, "f1": f1, "n_flagged": len(ids), "n_fake": n_fake, "true_positives": tp}
