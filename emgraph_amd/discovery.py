"""Discovery on the GPU: nearest neighbours, duplicate detection, clustering and discovered facts (AmpliGraph 1.x's
``find_nearest_neighbours``, ``find_duplicates``, ``find_clusters`` and ``discover_facts``), without the embedding tables ever
leaving the device.

DISTANCES (the contract; include/emgraph_hip.h).  Rows are embeddings as ``get_embeddings`` returns them
(ComplEx / HolE: the whole 2k row); no link function and no FocusE weight applies.
  euclidean / l2   sqrtf of the k-ordered f32 chain fmaf(d, d, acc), d = a_k - b_k: the bits of the negated TransE-L2 score
                   of the exact 1-vs-all kernels for the same two rows;
  cosine           1 - dot, dot the k-ordered f32 chain fmaf(a_k, b_k, acc) over rows normalised beforehand (every element
                   divided by sqrtf of the row's chain sum of squares; an all-zero row stays zero: its distance is 1).

Nearest neighbours are the fused score-and-select kernel of top-N completions (emg_eval_topn) with the query rows handed in
directly; duplicates are the radius join emg_rows_within (csrc/emg_neigh.hip); clusters are an exact DBSCAN on the same
join (emg_rows_dbscan, csrc/emg_cluster.hip) or the k-means estimator ``KMeans`` (emg_rows_kmeans, csrc/emg_kmeans.hip).  Discovered facts rank a grid of candidate triples of a relation with one
1-vs-all row per grid row and column, each counted against many thresholds (emg_eval_grid_count, csrc/emg_grid.hip; DESIGN.md
4.4 "Discovered facts").  Every argument is validated before the device is asked for.
"""
from __future__ import annotations

import logging
import math
from fractions import Fraction

import numpy as np

from . import _lib as L
from .evaluation.protocol import _UNSEEN_MSG, _lookup_labels, idx_to_labels, to_idx

logger = logging.getLogger(__name__)

_NN_METRICS = {"euclidean": L.METRIC_L2, "cosine": L.METRIC_COSINE}
_DUP_METRICS = {"l2": L.METRIC_L2, "cosine": L.METRIC_COSINE}
_MODES = ("entity", "relation", "triple")
QUERY_CHUNK = 4096   # query rows per emg_eval_topn launch (as ranking.topn_device)


def _require_fitted(model):
    if not model.is_fitted:
        msg = "Model has not been fitted."
        logger.error(msg)
        raise RuntimeError(msg)


def _ids_of(labels, mapping, concept_type, from_idx):
    labels = np.asarray(labels).reshape(-1)
    if not from_idx:
        return _lookup_labels(labels, mapping, concept_type)
    if labels.size and labels.dtype.kind not in "iu":
        raise ValueError("from_idx=True needs integer ids")
    ids = labels.astype(np.int64)
    if ids.size and not ((ids >= 0) & (ids < len(mapping))).all():
        raise ValueError(_UNSEEN_MSG.format(concept_type=concept_type))
    return ids


# ---- pure helpers (no device) --------------------------------------------------------------------
def neighbourhoods(pairs, n, labels=None):
    """The result of find_duplicates from the join's pairs: ``pairs`` holds (i << 32 | j) for every ordered pair of
    different rows i, j < n within the tolerance.  With N(i) = {i} + {j : (i, j) in pairs} the result is
    {frozenset(N(i)) : |N(i)| > 1} — neighbourhoods, not connected components: a ~ b ~ c with a and c apart gives {a, b},
    {a, b, c} and {b, c}.  ``labels[i]`` (default: i itself) is what the sets hold."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1)
    i, j = pairs >> 32, pairs & 0xffffffff
    if pairs.size and not ((i >= 0) & (i < n) & (j < n) & (i != j)).all():
        raise ValueError("a pair names a row outside [0, %d) or a row with itself" % n)
    order = np.lexsort((j, i))
    i, j = i[order], j[order]
    rows, starts = np.unique(i, return_index=True)
    ends = np.append(starts[1:], len(i))
    name = (lambda r: r) if labels is None else (lambda r: labels[r])
    out = set()
    for r, a, b in zip(rows.tolist(), starts.tolist(), ends.tolist()):
        out.add(frozenset([name(r)] + [name(c) for c in j[a:b].tolist()]))
    return out


def auto_tolerance(nn_dist, expected_fraction_duplicates):
    """The smallest tolerance at which at least ``expected_fraction_duplicates`` of the rows have another row within it: the
    ceil(f n)-th smallest entry of ``nn_dist`` (each row's distance to its nearest other row, +inf where there is none).
    f is read as the decimal number it was written as (0.1 of 30 rows is 3 rows, not 4).  ValueError if fewer rows than
    that have a neighbour at all."""
    d = np.asarray(nn_dist, dtype=np.float32).reshape(-1)
    f = float(expected_fraction_duplicates)
    if not 0.0 < f <= 1.0:
        raise ValueError("expected_fraction_duplicates must be in (0, 1], got %r" % (expected_fraction_duplicates,))
    if d.size == 0:
        raise ValueError("tolerance='auto' needs at least two rows")
    m = max(1, math.ceil(Fraction(repr(f)) * d.size))
    tol = np.sort(d)[m - 1]   # (a NaN sorts last)
    if not np.isfinite(tol):
        raise ValueError("tolerance='auto': only %d of %d rows have a nearest other row, %d are asked for"
                         % (int(np.isfinite(d).sum()), d.size, m))
    return float(tol)


def _check_n_neighbors(n_neighbors):
    if isinstance(n_neighbors, bool) or not isinstance(n_neighbors, (int, np.integer)) or not 1 <= int(n_neighbors) <= L.TOPN_MAX:
        raise ValueError("n_neighbors must be an integer in [1, %d] (EMG_TOPN_MAX), got %r" % (L.TOPN_MAX, n_neighbors))
    return int(n_neighbors)


# ---- nearest neighbours -----------------------------------------------------------------------------
def neighbours_device(ent, k_int, query_ids, n_neighbors, metric, entities_subset=None):
    """(ids int32 [n, n_neighbors] padded with -1, distances float32 padded with +inf) of the rows ``query_ids`` of the
    device table ``ent`` among all its rows or ``entities_subset``.  The selection is emg_eval_topn's (a sibling of
    ranking.topn_device: the query rows are table rows, not built from triples): TransE-L2 on the rows gives -distance,
    DistMult on the normalised copies gives dot."""
    import torch

    from . import device as D
    q = torch.from_numpy(np.asarray(query_ids, dtype=np.int64)).to(ent.device)
    cand, n_cand = None, int(ent.shape[0])
    if entities_subset is not None:
        sub = np.unique(np.asarray(entities_subset, dtype=np.int64))   # de-duplicated, ascending
        cand, n_cand = torch.from_numpy(sub.astype(np.int32)).to(ent.device), len(sub)
    table = ent if metric == L.METRIC_L2 else D.rows_normalize(ent, k_int)
    model_id = L.TRANSE_L2 if metric == L.METRIC_L2 else L.DISTMULT
    ws, pending = None, []
    for c0 in range(0, q.numel(), QUERY_CHUNK):
        Q = table.index_select(0, q[c0:c0 + QUERY_CHUNK])
        if ws is None:   # one workspace: the launches are ordered on the stream and the first tile is the largest
            ws = torch.empty(D.eval_topn_ws_bytes(Q.shape[0], n_cand, n_neighbors), dtype=torch.uint8, device=ent.device)
        pending.append(D.eval_topn(model_id, Q, table, k_int, 1.0, n_neighbors, cand=cand, ws=ws))
    if not pending:
        return np.zeros((0, n_neighbors), np.int32), np.zeros((0, n_neighbors), np.float32)
    ids = torch.cat([p[0] for p in pending]).cpu().numpy()
    scores = torch.cat([p[1] for p in pending]).cpu().numpy()
    if metric == L.METRIC_L2:
        return ids, -scores   # padding: -(-inf)
    # 1 - dot rounds different dots onto one distance: put each row in (distance, id) order (the selection itself is by dot)
    dist = np.where(ids < 0, np.float32(np.inf), np.float32(1.0) - scores).astype(np.float32)
    key_id = np.where(ids < 0, np.iinfo(np.int32).max, ids)
    order = np.lexsort((key_id, dist), axis=1)
    return np.take_along_axis(ids, order, axis=1), np.take_along_axis(dist, order, axis=1)


def find_nearest_neighbours(model, entities, n_neighbors=10, entities_subset=None, metric="euclidean", from_idx=False):
    """The ``n_neighbors`` entities closest to each of ``entities`` in embedding space, among all entities or
    ``entities_subset``.  The query entity is a candidate like any other (at distance 0 it comes first if it is among the
    candidates), as scikit-learn's ``kneighbors`` on the fitted set gives it.

    Returns ``(neighbours [n, n_neighbors], distances float32 [n, n_neighbors])`` in ascending distance, equal distances by
    ascending entity id; ``neighbours`` is an object array of labels (int32 ids with ``from_idx=True``).  With fewer
    candidates than ``n_neighbors`` a row is padded with None (id -1) and +inf.  ``metric``: 'euclidean' or 'cosine' (the
    module's distance definitions).

    'cosine': WHICH candidates a row holds is decided on the device by ``dot`` (descending, equal dots by ascending id); the
    row is then put into (distance, id) order.  ``1 - dot`` can round two different dots onto one distance, so at the last
    position a candidate with that same rounded distance and a lower id, but a dot smaller in its last bits, can be the one
    left out.  'euclidean' has no such case: selection and order use the same value."""
    n_neighbors = _check_n_neighbors(n_neighbors)
    if metric not in _NN_METRICS:
        raise ValueError("metric must be 'euclidean' or 'cosine', got %r" % (metric,))
    _require_fitted(model)
    ids = _ids_of(entities, model.ent_to_idx, "entities", from_idx)
    subset = None if entities_subset is None else _ids_of(entities_subset, model.ent_to_idx, "entities", from_idx)
    ent, _ = model._device_tables()
    nbr, dist = neighbours_device(ent, model.internal_k, ids, n_neighbors, _NN_METRICS[metric], subset)
    return (nbr if from_idx else idx_to_labels(nbr, model.ent_to_idx)), dist


# ---- duplicates -----------------------------------------------------------------------------------
def duplicates_device(table, k_int, metric, tolerance, expected_fraction_duplicates=0.1):
    """(packed pairs int64 on the host, tolerance) of the self-join of the device table ``table`` [n, k_int].  With
    ``tolerance`` None it is auto_tolerance of one pass that finds every row's nearest other row.  The pair pass runs at
    most twice: if the first buffer (4 n entries) was too small, the second is sized from the counts the first pass left.
    Every pass is a full n x n join: two at most with a given tolerance, three at most with the automatic one (the
    tolerance is not known while the first runs, so that pass cannot collect pairs)."""
    import torch

    from . import device as D
    n = int(table.shape[0])
    rows = D.rows_normalize(table, k_int) if metric == L.METRIC_COSINE else table
    if tolerance is None:
        _, nn_dist, _, _, _ = D.rows_within(metric, rows, rows, k_int, 0, 0.0)
        tolerance = auto_tolerance(nn_dist.cpu().numpy(), expected_fraction_duplicates)
    tolerance = float(np.float32(tolerance))
    cap = max(1024, 4 * n)
    count, _, _, pairs, pc = D.rows_within(metric, rows, rows, k_int, 0, tolerance, pairs_capacity=cap)
    written, overflow = pc.cpu().tolist()
    if overflow:
        cap = int(count.sum(dtype=torch.int64).item())
        _, _, _, pairs, pc = D.rows_within(metric, rows, rows, k_int, 0, tolerance, pairs_capacity=cap)
        written, overflow = pc.cpu().tolist()
        if overflow or written != cap:
            raise L.EmgError("emg_rows_within: %d pairs counted, %d written" % (cap, written))
    return pairs[:written].cpu().numpy(), tolerance


def _dedupe(rows):
    """indices of the first occurrences, in order (a label compared with itself is no duplicate)"""
    seen = {}
    for i, r in enumerate(rows.tolist()):
        seen.setdefault(tuple(r) if isinstance(r, list) else r, i)
    return np.fromiter(seen.values(), dtype=np.int64, count=len(seen))


def find_duplicates(X, model, mode="entity", metric="l2", tolerance="auto", expected_fraction_duplicates=0.1, verbose=False):
    """Groups of entities, relations or triples of ``X`` whose embeddings lie within ``tolerance`` of each other.

    ``X``: the labels to compare, [n] for ``mode`` 'entity' / 'relation', [n, 3] for 'triple' (a triple's embedding is the
    concatenation of its subject, predicate and object rows); a label given twice is compared once.  ``metric``: 'l2' or
    'cosine'.  With N(i) the rows within the tolerance of row i, i included, the result is {frozenset(N(i)) : |N(i)| > 1}
    — neighbourhoods, as AmpliGraph returns them, not connected components.  ``tolerance='auto'``: the smallest tolerance
    at which at least ``expected_fraction_duplicates`` of the rows have another row within it — the exact quantile of the
    rows' nearest-other distances from one device pass (AmpliGraph searches for it iteratively).

    Returns ``(duplicates, tolerance)``: a set of frozensets of labels (of (s, p, o) tuples for triples), and the tolerance
    used."""
    if mode not in _MODES:
        raise ValueError("mode must be one of %r, got %r" % (_MODES, mode))
    if metric not in _DUP_METRICS:
        raise ValueError("metric must be 'l2' or 'cosine', got %r" % (metric,))
    if isinstance(tolerance, str):
        if tolerance != "auto":
            raise ValueError("tolerance must be 'auto' or a non-negative number, got %r" % (tolerance,))
        f = expected_fraction_duplicates
        if isinstance(f, bool) or not isinstance(f, (int, float, np.integer, np.floating)) or not 0.0 < float(f) <= 1.0:
            raise ValueError("expected_fraction_duplicates must be in (0, 1], got %r" % (f,))
        tol = None
    else:
        if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float, np.integer, np.floating)) \
                or not 0.0 <= float(tolerance) < float("inf"):
            raise ValueError("tolerance must be 'auto' or a non-negative number, got %r" % (tolerance,))
        tol = float(tolerance)
    _require_fitted(model)
    X = np.asarray(X)
    if mode == "triple":
        if X.ndim == 1 and X.shape[0] == 3:
            X = X[np.newaxis, :]
        if X.ndim != 2 or X.shape[1] != 3:
            raise ValueError("X must have shape [n, 3] for mode='triple'")
        X = X[_dedupe(X)]
        idx = to_idx(X, ent_to_idx=model.ent_to_idx, rel_to_idx=model.rel_to_idx) if len(X) else np.zeros((0, 3), np.int64)
        labels = [tuple(t) for t in X.tolist()]
    else:
        if X.ndim != 1:
            raise ValueError("X must have shape [n] for mode=%r" % mode)
        X = X[_dedupe(X)]
        mapping, concept = (model.ent_to_idx, "entities") if mode == "entity" else (model.rel_to_idx, "relations")
        idx = _lookup_labels(X, mapping, concept) if len(X) else np.zeros(0, np.int64)
        labels = X.tolist()
    n = len(labels)
    if n < 2:
        if tol is None:
            raise ValueError("tolerance='auto' needs at least two rows")
        return set(), tol

    import torch
    ent, rel = model._device_tables()
    k_int = model.internal_k
    it = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(ent.device)
    if mode == "triple":   # the gather is a copy; the distances are the library's
        table = torch.cat([ent.index_select(0, it[:, 0]), rel.index_select(0, it[:, 1]), ent.index_select(0, it[:, 2])], dim=1)
        k_int = 3 * k_int
    else:
        table = (ent if mode == "entity" else rel).index_select(0, it)
    pairs, tol = duplicates_device(table, k_int, _DUP_METRICS[metric], tol, expected_fraction_duplicates)
    if verbose:
        logger.info("find_duplicates: tolerance %g, %d pairs among %d rows", tol, len(pairs) // 2, n)
    return neighbourhoods(pairs, n, labels), tol


# ---- clusters -------------------------------------------------------------------------------------
_CLUSTER_DEFAULTS = {"eps": 0.5, "min_samples": 5, "metric": "l2"}


def _gather_rows(X, model, mode):
    """(idx, gather) of the labels ``X`` — checked against the model's mappings on the host; ``gather()`` asks for the device
    and returns (table [len(X), k], k): the rows in the order of X, NOT de-duplicated."""
    X = np.asarray(X)
    if mode == "triple":
        if X.ndim == 1 and X.shape[0] == 3:
            X = X[np.newaxis, :]
        if X.ndim != 2 or X.shape[1] != 3:
            raise ValueError("X must have shape [n, 3] for mode='triple'")
        idx = to_idx(X, ent_to_idx=model.ent_to_idx, rel_to_idx=model.rel_to_idx) if len(X) else np.zeros((0, 3), np.int64)
    else:
        if X.ndim != 1:
            raise ValueError("X must have shape [n] for mode=%r" % mode)
        mapping, concept = (model.ent_to_idx, "entities") if mode == "entity" else (model.rel_to_idx, "relations")
        idx = _lookup_labels(X, mapping, concept) if len(X) else np.zeros(0, np.int64)

    def gather():
        import torch
        ent, rel = model._device_tables()
        k_int = model.internal_k
        it = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(ent.device)
        if mode == "triple":   # the gather is a copy; the distances are the library's
            return torch.cat([ent.index_select(0, it[:, 0]), rel.index_select(0, it[:, 1]), ent.index_select(0, it[:, 2])],
                             dim=1), 3 * k_int
        return (ent if mode == "entity" else rel).index_select(0, it), k_int
    return idx, gather


def _is_device_tensor(rows):
    return type(rows).__module__.split(".")[0] == "torch" and hasattr(rows, "is_cuda")


class KMeans:
    """Lloyd's k-means on the device, with scikit-learn's interface: ``KMeans(n_clusters=6, n_init=50, max_iter=500)`` is what
    AmpliGraph's ``find_clusters`` example passes as ``clustering_algorithm``, and find_clusters hands an instance of THIS
    class the gathered device table without a host copy.

    Names and defaults are ``sklearn.cluster.KMeans``'; ``seed`` (an int >= 0) stands in for ``random_state``.  ``init``:
    'k-means++', 'random' or an array [n_clusters, width]; ``n_init='auto'``: 1 for 'k-means++' or an array, 10 for 'random'.
    Restart r draws from ``np.random.default_rng([seed, r])``: 'k-means++' the first row (``rng.integers(n)``) and then
    ``rng.random(n_clusters - 1)``, 'random' ``rng.choice(n, n_clusters, replace=False)``.  The run with the lowest inertia is
    kept, the earliest on ties.

    SCOPE: Euclidean only — no sample weights, no cosine k-means.  The arithmetic is pinned (include/emgraph_hip.h, DESIGN.md
    4.4 "k-means"): distances are the module's l2 chain, a row equally near two centres takes the lower index, means and
    inertia are f64 sums in a fixed order, so two runs give the same bits.  Two deviations from scikit-learn: an empty
    cluster keeps its centre (scikit-learn relocates it), and 'k-means++' is plain D^2 sampling (scikit-learn tries several
    candidates per pick).  A row holding a NaN gets label -1.

    After ``fit``: ``labels_`` (int32 [n]), ``cluster_centers_`` (float32 [n_clusters, width]), ``inertia_`` (float),
    ``n_iter_`` (the updates of the kept run), ``n_restarts_`` (the runs made) — all on the host."""

    def __init__(self, n_clusters=8, *, init="k-means++", n_init="auto", max_iter=300, tol=1e-4, seed=0):
        if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)) \
                or not 1 <= int(n_clusters) <= np.iinfo(np.int32).max:
            raise ValueError("n_clusters must be an integer >= 1, got %r" % (n_clusters,))
        if isinstance(init, str):
            if init not in ("k-means++", "random"):
                raise ValueError("init must be 'k-means++', 'random' or an array [n_clusters, width], got %r" % (init,))
        else:
            try:
                arr = np.array(init, dtype=np.float32, order="C", copy=True)
            except (TypeError, ValueError):
                raise ValueError("init must be 'k-means++', 'random' or an array [n_clusters, width], got %r" % (init,)) from None
            if isinstance(init, bool) or arr.ndim != 2 or arr.shape[0] != int(n_clusters) or arr.shape[1] < 1:
                raise ValueError("init must be 'k-means++', 'random' or an array [n_clusters, width]; got the shape %r for "
                                 "n_clusters = %d" % (arr.shape, int(n_clusters)))
            init = arr
        if isinstance(n_init, str):
            if n_init != "auto":
                raise ValueError("n_init must be 'auto' or an integer >= 1, got %r" % (n_init,))
        elif isinstance(n_init, bool) or not isinstance(n_init, (int, np.integer)) or int(n_init) < 1:
            raise ValueError("n_init must be 'auto' or an integer >= 1, got %r" % (n_init,))
        if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) \
                or not 1 <= int(max_iter) <= np.iinfo(np.int32).max:
            raise ValueError("max_iter must be an integer >= 1, got %r" % (max_iter,))
        if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) \
                or not 0.0 <= float(tol) < float("inf"):
            raise ValueError("tol must be a finite number >= 0, got %r" % (tol,))
        self.n_clusters = int(n_clusters)
        self.init = init
        self.n_init = n_init if isinstance(n_init, str) else int(n_init)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.seed = _check_seed(seed)

    def _restarts(self):
        if self.n_init != "auto":
            return self.n_init
        return 10 if isinstance(self.init, str) and self.init == "random" else 1

    def _check_rows(self, rows, fitting):
        """the shape checks of fit / predict, before the device is asked for: (rows, n, width)"""
        if _is_device_tensor(rows):
            import torch
            if not (rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2 and (rows.shape[1] == 0 or rows.stride(1) == 1)):
                raise ValueError("rows must be a float32 ndarray [n, width] or a 2-D float32 device tensor with unit column stride")
        else:
            rows = np.asarray(rows)
            if rows.ndim != 2 or rows.dtype != np.float32:
                raise ValueError("rows must be a float32 ndarray [n, width] or a device tensor, got %s of shape %r"
                                 % (rows.dtype, rows.shape))
        n, width = int(rows.shape[0]), int(rows.shape[1])
        if width < 1:
            raise ValueError("rows must have at least one column")
        if fitting:
            if n < self.n_clusters:
                raise ValueError("n_samples=%d should be >= n_clusters=%d." % (n, self.n_clusters))
            if not isinstance(self.init, str) and self.init.shape[1] != width:
                raise ValueError("init has %d columns, the rows have %d" % (self.init.shape[1], width))
        else:
            if not hasattr(self, "cluster_centers_"):
                raise RuntimeError("This KMeans instance is not fitted yet.")
            if self.cluster_centers_.shape[1] != width:
                raise ValueError("the rows have %d columns, the fitted centres %d" % (width, self.cluster_centers_.shape[1]))
            if n < 1:
                raise ValueError("rows must hold at least one row")
        return rows, n, width

    @staticmethod
    def _on_device(rows):
        import torch

        from . import device as D
        if _is_device_tensor(rows):
            return rows
        D.require_gpu()
        return torch.from_numpy(np.ascontiguousarray(rows)).cuda()

    def fit(self, rows):
        """Cluster the rows (a float32 ndarray [n, width] or a device tensor); ``n < n_clusters`` raises ValueError."""
        rows, n, width = self._check_rows(rows, fitting=True)
        import torch

        from . import device as D
        X = self._on_device(rows)
        dev, C = X.device, self.n_clusters
        ws = torch.empty(D.rows_kmeans_ws_bytes(n, C, width), dtype=torch.uint8, device=dev)
        best = None
        restarts = self._restarts()
        for r in range(restarts):
            rng = np.random.default_rng([self.seed, r])
            if not isinstance(self.init, str):
                centres = torch.from_numpy(self.init).to(dev)
            elif self.init == "random":
                pick = torch.from_numpy(rng.choice(n, C, replace=False).astype(np.int64)).to(dev)
                centres = X.index_select(0, pick).contiguous()
            else:
                first = int(rng.integers(n))
                centres, _ = D.rows_kmeans_seed(X, width, C, first, rng.random(C - 1), ws=ws)
            labels, info = D.rows_kmeans(X, width, centres, self.max_iter, self.tol, ws=ws)
            inertia, n_iter, _, _ = D.kmeans_info(info)   # the one host read of the run
            if best is None or inertia < best[0]:
                best = (inertia, n_iter, labels, centres)
        self.inertia_, self.n_iter_ = best[0], best[1]
        self.labels_ = best[2].cpu().numpy()
        self.cluster_centers_ = best[3].cpu().numpy()
        self.n_restarts_ = restarts
        return self

    def fit_predict(self, rows):
        """``fit(rows).labels_``: int32 [n] on the host"""
        return self.fit(rows).labels_

    def predict(self, rows):
        """The label of each row under the fitted centres (the assignment rule of fit): int32 [n] on the host"""
        rows, n, width = self._check_rows(rows, fitting=False)
        import torch

        from . import device as D
        X = self._on_device(rows)
        centres = torch.from_numpy(np.ascontiguousarray(self.cluster_centers_)).to(X.device)
        labels, _ = D.rows_kmeans(X, width, centres, 0, 0.0)
        return labels.cpu().numpy()


def find_clusters(X, model, clustering_algorithm="dbscan", mode="entity", *, eps=0.5, min_samples=5, metric="l2"):
    """Cluster the embeddings of the entities, relations or triples ``X``; returns an int32 array [len(X)] of cluster labels
    in the order of ``X``.

    ``X``: [n] labels for ``mode`` 'entity' / 'relation', [n, 3] for 'triple' (the s, p and o rows concatenated).  Rows are
    NOT de-duplicated: a label given twice is two rows, and it changes the density exactly as it would in scikit-learn.

    ``clustering_algorithm="dbscan"`` (the default) runs an exact DBSCAN on the device (emg_rows_dbscan): with N(i) the rows
    within ``eps`` of row i (the module's ``metric`` 'l2' or 'cosine', d <= eps, i included), row i is core iff
    |N(i)| >= ``min_samples``; clusters are the connected components of the core rows, numbered from 0 in ascending order of
    their lowest core row; a row that is not core takes the lowest label among the core rows within eps of it, -1 (noise) if
    there is none — the labels of ``sklearn.cluster.DBSCAN(eps, min_samples).fit_predict``.

    Any object with a ``fit_predict`` method (AmpliGraph's calling convention: a scikit-learn clusterer) gets the rows,
    gathered on the device and copied to the host once, and ``np.asarray(obj.fit_predict(rows))`` is returned as it is; ``eps``,
    ``min_samples`` and ``metric`` belong to the device path and must then be left at their defaults.

    An instance of this module's ``KMeans`` is such an object whose rows STAY on the device: it gets the gathered device
    table (no host copy) and its ``labels_`` come back as int32 on the host; fewer rows than ``n_clusters`` raise ValueError
    before the device is asked for."""
    if mode not in _MODES:
        raise ValueError("mode must be one of %r, got %r" % (_MODES, mode))
    on_device = isinstance(clustering_algorithm, str)
    if on_device:
        if clustering_algorithm != "dbscan":
            raise ValueError("clustering_algorithm must be 'dbscan' or an object with a fit_predict method, got %r"
                             % (clustering_algorithm,))
        if metric not in _DUP_METRICS:
            raise ValueError("metric must be 'l2' or 'cosine', got %r" % (metric,))
        if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) \
                or not 0.0 <= float(eps) < float("inf"):
            raise ValueError("eps must be a finite number >= 0, got %r" % (eps,))
        if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) \
                or not 1 <= int(min_samples) <= np.iinfo(np.int32).max:
            raise ValueError("min_samples must be an integer >= 1, got %r" % (min_samples,))
    else:
        if not callable(getattr(clustering_algorithm, "fit_predict", None)):
            raise ValueError("clustering_algorithm must be 'dbscan' or an object with a fit_predict method, got %r"
                             % (clustering_algorithm,))
        given = {"eps": eps, "min_samples": min_samples, "metric": metric}
        changed = sorted(name for name, v in given.items()
                         if type(v) is not type(_CLUSTER_DEFAULTS[name]) or v != _CLUSTER_DEFAULTS[name])
        if changed:
            raise ValueError("%s belong(s) to clustering_algorithm='dbscan'; set the parameters of %r on the object itself"
                             % (", ".join(changed), type(clustering_algorithm).__name__))
    _require_fitted(model)
    idx, gather = _gather_rows(X, model, mode)
    if on_device and len(idx) == 0:
        return np.zeros(0, np.int32)
    own_kmeans = isinstance(clustering_algorithm, KMeans)
    if own_kmeans and len(idx) < clustering_algorithm.n_clusters:
        raise ValueError("n_samples=%d should be >= n_clusters=%d." % (len(idx), clustering_algorithm.n_clusters))

    table, k_int = gather()
    if own_kmeans:
        return np.asarray(clustering_algorithm.fit_predict(table[:, :k_int]), dtype=np.int32)
    if not on_device:
        return np.asarray(clustering_algorithm.fit_predict(table[:, :k_int].cpu().numpy()))
    from . import device as D
    code = _DUP_METRICS[metric]
    rows = D.rows_normalize(table, k_int) if code == L.METRIC_COSINE else table
    labels, _, _ = D.rows_dbscan(rows, k_int, code, float(np.float32(eps)), int(min_samples))
    return labels.cpu().numpy()


# ---- discovered facts -----------------------------------------------------------------------------
STRATEGIES = ("random_uniform", "entity_frequency", "graph_degree", "cluster_coefficient", "cluster_triangles", "exhaustive")


def _check_strategy(strategy):
    if strategy == "cluster_squares":
        raise ValueError("strategy 'cluster_squares' is not available: nothing here pins its definition (networkx's "
                         "square_clustering is not on the host path); use one of %r" % (STRATEGIES,))
    if strategy not in STRATEGIES:
        raise ValueError("strategy must be one of %r, got %r" % (STRATEGIES, strategy))
    return strategy


def _check_max_candidates(max_candidates, n_ent):
    """the number of cells a grid may hold: an int >= 1, or a float in (0, 1] meaning that share of |E|^2"""
    m = max_candidates
    if isinstance(m, (int, np.integer)) and not isinstance(m, bool) and int(m) >= 1:
        return int(m)
    if isinstance(m, (float, np.floating)) and 0.0 < float(m) <= 1.0:
        cells = int(float(m) * n_ent * n_ent)
        if cells >= 1:
            return cells
    raise ValueError("max_candidates must be an integer >= 1 or a float in (0, 1] that leaves at least one of the |E|^2 "
                     "cells, got %r" % (max_candidates,))


def _check_discover_top_n(top_n):
    if isinstance(top_n, bool) or not isinstance(top_n, (int, np.integer)) or int(top_n) < 1:
        raise ValueError("top_n must be a positive integer, got %r" % (top_n,))
    return int(top_n)


def _check_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or int(seed) < 0:
        raise ValueError("seed must be a non-negative integer, got %r" % (seed,))
    return int(seed)


def strategy_weights(X_idx, n_ent, strategy):
    """float64 [n_ent]: the weight with which ``strategy`` draws each entity, from the int triples ``X_idx`` (all relations).
    The graph strategies use the undirected simple graph of the (s, o) pairs: parallel edges and both directions count once,
    self-loops not at all.  ValueError when every weight is zero."""
    _check_strategy(strategy)
    X_idx = np.asarray(X_idx, dtype=np.int64).reshape(-1, 3)
    if strategy in ("random_uniform", "exhaustive"):
        w = np.ones(n_ent, np.float64)
    elif strategy == "entity_frequency":
        w = np.bincount(np.concatenate([X_idx[:, 0], X_idx[:, 2]]), minlength=n_ent).astype(np.float64)
    else:
        import scipy.sparse as sp
        s, o = X_idx[:, 0], X_idx[:, 2]
        keep = s != o
        s, o = s[keep], o[keep]
        A = sp.coo_matrix((np.ones(2 * len(s), np.int64), (np.concatenate([s, o]), np.concatenate([o, s]))),
                          shape=(n_ent, n_ent)).tocsr()
        A.data[:] = 1   # (tocsr summed the repeats)
        deg = np.asarray(A.sum(axis=1)).reshape(-1).astype(np.float64)
        if strategy == "graph_degree":
            w = deg
        else:
            tri = np.asarray((A @ A).multiply(A).sum(axis=1)).reshape(-1).astype(np.float64) / 2.0   # closed 3-walks / 2
            if strategy == "cluster_triangles":
                w = tri
            else:
                pairs = deg * (deg - 1.0)
                w = np.divide(2.0 * tri, pairs, out=np.zeros(n_ent, np.float64), where=pairs > 0)
    if not (w > 0).any():
        raise ValueError("strategy %r gives every entity the weight zero on this graph" % (strategy,))
    return w


def _grid_of(weights, strategy, rel_id, max_cells, seed):
    n_ent = len(weights)
    if strategy == "exhaustive":
        ids = np.arange(n_ent, dtype=np.int64)
        return ids, ids.copy()
    eligible = int((weights > 0).sum())
    n_s = min(math.isqrt(max_cells), eligible)
    n_o = min(max_cells // n_s, eligible)
    p = weights / weights.sum()
    rng = np.random.default_rng([seed, rel_id])
    S = rng.choice(n_ent, size=n_s, replace=False, p=p)
    O = rng.choice(n_ent, size=n_o, replace=False, p=p)
    return np.sort(S).astype(np.int64), np.sort(O).astype(np.int64)


def generate_candidates(X, model, strategy, target_rel, max_candidates, seed=0):
    """The candidate grid of ONE relation: ``(S, O)``, ascending int64 entity ids — the candidates are the cells
    (s, target_rel, o), s in S, o in O, that are not in ``X`` (the caller drops those).

    ``strategy`` weighs the entities (strategy_weights, from all of ``X``); S and then O are drawn WITHOUT replacement by
    ``np.random.default_rng([seed, rel_id]).choice(|E|, size, replace=False, p=weights / sum)``: a zero-weight entity is never
    drawn.  ``max_candidates`` (an int, or a float in (0, 1]: that share of |E|^2) bounds the cells: |S| =
    min(floor(sqrt(max_candidates)), eligible), |O| = min(max_candidates // |S|, eligible), eligible the entities of non-zero
    weight.  'exhaustive': S = O = every entity, no sampling, ``max_candidates`` ignored.  Runs on the host."""
    _check_strategy(strategy)
    seed = _check_seed(seed)
    _require_fitted(model)
    n_ent = len(model.ent_to_idx)
    if strategy != "exhaustive":
        max_candidates = _check_max_candidates(max_candidates, n_ent)
    rel_id = int(_lookup_labels(np.asarray([target_rel]), model.rel_to_idx, "relations")[0])
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != 3:
        raise ValueError("X must have shape [n, 3]")
    X_idx = to_idx(X, ent_to_idx=model.ent_to_idx, rel_to_idx=model.rel_to_idx) if len(X) else np.zeros((0, 3), np.int64)
    return _grid_of(strategy_weights(X_idx, n_ent, strategy), strategy, rel_id, max_candidates, seed)


def discover_facts(X, model, top_n=10, strategy="random_uniform", max_candidates=100, target_rel=None, seed=0):
    """Triples that are not in ``X`` and that the model ranks near the top (AmpliGraph 1.x's ``discover_facts``).

    For every relation of the model (or ``target_rel``: a label or a list of labels) the grid of generate_candidates is
    ranked against ALL corruptions on both sides, ``X`` being the filter — the ranks evaluate_performance(cells, model,
    filter_triples=X, corrupt_side='s,o') gives with the 'worst' strategy — and a cell that is not in ``X`` is kept when
    (subject rank + object rank) / 2 <= ``top_n`` (any positive int).  The grid needs |S| + |O| rows of 1-vs-all scoring, not
    2 |S| |O| (ranking.grid_ranks_device, csrc/emg_grid.hip).

    Returns ``(triples [m, 3] of labels, average ranks float64 [m])``: relations in the order asked for (the model's id order
    without ``target_rel``), the cells of a relation by (subject id, object id); shapes (0, 3) and (0,) when nothing is found.
    Every argument is validated before the device is asked for."""
    top_n = _check_discover_top_n(top_n)
    _check_strategy(strategy)
    seed = _check_seed(seed)
    _require_fitted(model)
    n_ent = len(model.ent_to_idx)
    max_cells = _check_max_candidates(max_candidates, n_ent) if strategy != "exhaustive" else None
    model._refuse_without_kernel("discover_facts")
    model._refuse_ranking_under_link("discover_facts", always=True)
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != 3:
        raise ValueError("X must have shape [n, 3]")
    X_idx = to_idx(X, ent_to_idx=model.ent_to_idx, rel_to_idx=model.rel_to_idx) if len(X) else np.zeros((0, 3), np.int64)
    X_idx = np.asarray(X_idx, dtype=np.int64)
    if target_rel is None:
        rel_ids = np.arange(len(model.rel_to_idx), dtype=np.int64)
    else:
        one = isinstance(target_rel, (str, bytes)) or np.ndim(target_rel) == 0
        wanted = np.asarray([target_rel] if one else target_rel).reshape(-1)
        rel_ids = _lookup_labels(wanted, model.rel_to_idx, "relations") if len(wanted) else np.zeros(0, np.int64)
    weights = strategy_weights(X_idx, n_ent, strategy)
    grids = [_grid_of(weights, strategy, int(r), max_cells, seed) for r in rel_ids]

    from .evaluation.ranking import FilterIndex, grid_ranks_device
    ent_labels = idx_to_labels(np.arange(n_ent), model.ent_to_idx)
    rel_labels = np.empty(len(model.rel_to_idx), dtype=object)
    for label, i in model.rel_to_idx.items():
        rel_labels[i] = label
    found, ranks = [], []
    if len(rel_ids):
        ent, rel = model._device_tables()
        findex = FilterIndex(X_idx)
    for r, (S, O) in zip(rel_ids.tolist(), grids):
        rank_s, rank_o = grid_ranks_device(model._model_id(), ent, rel, model.internal_k, model._scale(), r, S, O, findex)
        avg = (rank_s + rank_o) / 2.0
        mine = X_idx[X_idx[:, 1] == r]
        known = np.isin(S[:, None] * np.int64(n_ent) + O[None, :], mine[:, 0] * np.int64(n_ent) + mine[:, 2])
        si, oi = np.nonzero((avg <= top_n) & ~known)   # row-major: by subject id, then object id
        out = np.empty((len(si), 3), dtype=object)
        out[:, 0], out[:, 1], out[:, 2] = ent_labels[S[si]], rel_labels[r], ent_labels[O[oi]]
        found.append(out)
        ranks.append(avg[si, oi])
    if not found:
        return np.empty((0, 3), dtype=object), np.zeros(0, np.float64)
    return np.concatenate(found, axis=0), np.concatenate(ranks).astype(np.float64)
