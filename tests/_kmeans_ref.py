"""k-means from its contract (no device, no scikit-learn): the expected result of emg_rows_kmeans, emg_rows_kmeans_seed and
emgraph_amd.discovery.KMeans, restated from include/emgraph_hip.h / DESIGN.md 4.4 "k-means".

Distances are tests/_chain_ref.l2_chain (the module's l2 chain, to the bit).  Every sum the contract fixes the order of is an
explicit float64 loop in that order — never np.sum, which adds pairwise.  Besides the results the functions report MARGINS: how
far each decision was from going the other way, so that a test can tell a wrong result from an arithmetic coin toss."""
import numpy as np

from tests._chain_ref import l2_chain

F32, F64 = np.float32, np.float64
CHUNK = 256


def assign(X, centres):
    """(labels int32 [n], dist f32 [n], margin): label = the lowest j among the nearest centres, a NaN distance is no
    candidate, no candidate: (-1, +inf).  margin: the smallest relative gap (second - best) / second over the rows with two
    candidates or more (inf if there is none; 0 where two centres are exactly equally near)."""
    D = l2_chain(X, centres)
    n, C = D.shape
    labels = np.full(n, -1, np.int32)
    dist = np.full(n, np.inf, F32)
    margin = np.inf
    nan_rows = np.isnan(D).any(axis=1)
    plain = np.nonzero(~nan_rows)[0]
    if plain.size:                               # no NaN in the row: argmin returns the FIRST minimum, the lowest index
        Dp = D[plain]
        j = np.argmin(Dp, axis=1)
        labels[plain], dist[plain] = j, Dp[np.arange(len(plain)), j]
        if C > 1:
            two = np.sort(Dp, axis=1)[:, :2].astype(F64)
            with np.errstate(invalid="ignore", divide="ignore"):
                gap = np.where(two[:, 1] == two[:, 0], 0.0, (two[:, 1] - two[:, 0]) / two[:, 1])
            margin = min(margin, float(gap.min()))
    for i in np.nonzero(nan_rows)[0]:
        cand = np.nonzero(~np.isnan(D[i]))[0]
        if cand.size == 0:
            continue
        d = D[i, cand]
        j = cand[d == d.min()][0]                # cand ascends: the lowest index among the minima
        labels[i], dist[i] = j, D[i, j]
        if cand.size > 1:
            second = np.sort(d)[1]
            gap = 0.0 if second == d.min() else (float(second) - float(d.min())) / float(second)
            margin = min(margin, gap)
    return labels, dist, margin


def _chunked_sum(rows64):
    """the contract's order: chunks of 256 rows, each added row after row from 0.0; then the chunk sums one after the other"""
    total = np.zeros(rows64.shape[1], F64)
    for c0 in range(0, len(rows64), CHUNK):
        s = np.zeros(rows64.shape[1], F64)
        for r in range(c0, min(c0 + CHUNK, len(rows64))):
            s = s + rows64[r]                    # element-wise: one addition per column, in row order
        total = total + s
    return total


def update(X, labels, centres):
    """(new centres f32, counts): the mean of each cluster's members in ascending row order; an empty cluster keeps its centre"""
    X64 = np.asarray(X, F64)
    out = np.array(centres, dtype=F32, copy=True)
    counts = np.zeros(len(centres), np.int64)
    for j in range(len(centres)):
        members = np.nonzero(labels == j)[0]
        counts[j] = len(members)
        if len(members):
            out[j] = (_chunked_sum(X64[members]) / F64(len(members))).astype(F32)
    return out, counts


def inertia_of(labels, dist):
    s = 0.0
    for i in np.nonzero(labels >= 0)[0]:
        d = float(dist[i])
        s += d * d
    return s


def tolerance(X, tol):
    """tol * mean over columns of var(X): float64, two-pass, the sums in the order of the update (rows [0, n) as one cluster)"""
    X64 = np.asarray(X, F64)
    n, k = X64.shape
    mean = _chunked_sum(X64) / F64(n)
    dev = X64 - mean
    var = _chunked_sum(dev * dev) / F64(n)
    s = 0.0
    for col in range(k):
        s += float(var[col])
    return float(tol) * (s / float(k))


def shift_of(new, old, counts):
    """sum over the clusters that have members (an empty one kept its centre: it moved by 0, whatever its centre holds)"""
    d = (np.asarray(new, F64) - np.asarray(old, F64))[counts > 0]
    s = 0.0
    for v in (d * d).reshape(-1):
        s += float(v)
    return s


def lloyd(X, centres, max_iter, tol):
    """One Lloyd run from ``centres``.  Returns a dict: labels, centres, inertia, n_iter, converged, tol_abs, and the margins
    assign_margin (the smallest over all assignments made), stop_margin (|shift - tol_abs| / tol_abs at the stop that the
    shift decided, else None), stopped_by ('labels', 'tol' or 'max_iter'), min_count (the smallest cluster at any update)."""
    X = np.ascontiguousarray(X, dtype=F32)
    centres = np.array(centres, dtype=F32, copy=True)
    tol_abs = tolerance(X, tol) if max_iter > 0 else 0.0
    labels, dist, margin = assign(X, centres)
    n_iter, converged, stopped_by, stop_margin, min_count = 0, False, "max_iter", None, None
    near_tol = np.inf                            # the closest any shift that did NOT stop the run came to tol_abs
    for _ in range(max_iter):
        new, counts = update(X, labels, centres)
        min_count = int(counts.min()) if min_count is None else min(min_count, int(counts.min()))
        shift = shift_of(new, centres, counts)
        centres = new
        n_iter += 1
        new_labels, dist, m = assign(X, centres)
        margin = min(margin, m)
        same = np.array_equal(new_labels, labels)
        labels = new_labels
        rel = abs(shift - tol_abs) / tol_abs if tol_abs > 0 else (np.inf if shift > 0 else 0.0)
        if same:
            converged, stopped_by = True, "labels"
            break
        if shift <= tol_abs:                     # (a NaN tol_abs never stops)
            converged, stopped_by, stop_margin = True, "tol", rel
            break
        near_tol = min(near_tol, rel)
    return {"labels": labels, "centres": centres, "inertia": inertia_of(labels, dist), "n_iter": n_iter, "converged": converged,
            "tol_abs": tol_abs, "assign_margin": margin, "stop_margin": stop_margin, "near_tol": near_tol,
            "stopped_by": stopped_by, "min_count": min_count, "dist": dist}


def seed_weights(m):
    m64 = np.asarray(m, F64)
    return np.where(np.isfinite(m), m64 * m64, 0.0)


def pick(w, u):
    """(row, margin) of the contract's pick: S_i = P_s + r_i over segments of 256 rows, the first i with S_i > u S_n; the last
    row if there is none; floor(u n) if S_n == 0.  margin: the distance of u S_n from the nearer of S_pick and the S before
    it, relative to S_n (inf for S_n == 0)."""
    n = len(w)
    totals = []
    for s0 in range(0, n, CHUNK):
        run = 0.0
        for i in range(s0, min(s0 + CHUNK, n)):
            run += float(w[i])
        totals.append(run)
    total = 0.0
    for t in totals:
        total += t
    if not total > 0.0:
        return min(int(u * n), n - 1), np.inf
    target = u * total
    P, s = 0.0, 0
    while s < len(totals) - 1:
        nxt = P + totals[s]
        if nxt > target:
            break
        P, s = nxt, s + 1
    end = min((s + 1) * CHUNK, n)
    row, r, before, at = end - 1, 0.0, P, None
    for i in range(s * CHUNK, end):
        r += float(w[i])
        if P + r > target:
            row, at = i, P + r
            break
        before = P + r
    if at is None:
        return row, 0.0
    return row, min(at - target, target - before) / total


def seed(X, n_clusters, first_row, u):
    """k-means++ by plain D^2 sampling: (chosen int32 [C], centres f32 [C, k], the smallest pick margin)"""
    X = np.ascontiguousarray(X, dtype=F32)
    n = len(X)
    chosen = [int(first_row)]
    m = np.full(n, np.inf, F32)
    margin = np.inf
    for c in range(1, n_clusters):
        d = l2_chain(X, X[chosen[-1]][None, :])[:, 0]
        with np.errstate(invalid="ignore"):
            m = np.where(d < m, d, m).astype(F32)          # a NaN is no candidate
        row, g = pick(seed_weights(m), float(u[c - 1]))
        margin = min(margin, g)
        chosen.append(int(row))
    return np.asarray(chosen, np.int32), X[chosen].copy(), margin


def draws(seed_value, restart, n, n_clusters, init):
    """what restart ``restart`` of the estimator draws on the host"""
    rng = np.random.default_rng([seed_value, restart])
    if init == "random":
        return rng.choice(n, n_clusters, replace=False)
    first = int(rng.integers(n))
    return first, rng.random(n_clusters - 1)


def kmeans(X, n_clusters, init="k-means++", n_init="auto", max_iter=300, tol=1e-4, seed_value=0):
    """the estimator: n_init runs, the lowest inertia kept, the earliest on ties.  Returns (the kept run's dict with 'restart'
    added, the list of all inertias)."""
    X = np.ascontiguousarray(X, dtype=F32)
    if n_init == "auto":
        n_init = 10 if isinstance(init, str) and init == "random" else 1
    best, inertias = None, []
    for r in range(n_init):
        if not isinstance(init, str):
            start = np.asarray(init, F32)
        elif init == "random":
            start = X[draws(seed_value, r, len(X), n_clusters, init)]
        else:
            first, u = draws(seed_value, r, len(X), n_clusters, init)
            start = seed(X, n_clusters, first, u)[1]
        run = lloyd(X, start, max_iter, tol)
        run["restart"] = r
        inertias.append(run["inertia"])
        if best is None or run["inertia"] < best["inertia"]:
            best = run
    return best, inertias
