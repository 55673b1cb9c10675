"""DBSCAN from its definition (no device, no scikit-learn): the expected result of emg_rows_dbscan / find_clusters.

With N(i) the rows within eps of row i, i included (row i of the boolean matrix ``within``):
  core     row i is core iff |N(i)| >= min_samples;
  clusters the connected components of the core rows under ``within``, numbered 0, 1, ... in ascending order of their
           lowest core row — found by a breadth-first search over core rows, started from every unlabelled core row in
           index order;
  border   a row that is not core takes the MINIMUM label of the core rows in N(i);
  noise    -1 for every other row.
"""
import numpy as np


def dbscan_ref(within, min_samples):
    """(labels int32 [n], core bool [n]) from the symmetric boolean matrix ``within`` (diagonal True)"""
    within = np.asarray(within, dtype=bool)
    n = within.shape[0]
    assert within.shape == (n, n) and (within == within.T).all() and within.diagonal().all()
    core = within.sum(1) >= min_samples
    labels = np.full(n, -1, np.int32)
    cluster = 0
    for start in range(n):
        if not core[start] or labels[start] >= 0:
            continue
        labels[start] = cluster
        frontier = [start]
        while frontier:
            nxt = []
            for u in frontier:
                new = np.nonzero(within[u] & core & (labels < 0))[0]
                labels[new] = cluster
                nxt.extend(new.tolist())
            frontier = nxt
        cluster += 1
    for i in np.nonzero(~core)[0]:
        near = labels[within[i] & core]
        if near.size:
            labels[i] = near.min()
    return labels, core


def summary(labels, core):
    """(clusters, border rows, noise rows)"""
    labels = np.asarray(labels)
    return int(labels.max(initial=-1)) + 1, int(((labels >= 0) & ~np.asarray(core, bool)).sum()), int((labels < 0).sum())
