"""Negative sampling beyond the reference's fair coin and uniform replacement (protocol.py:598-641), host side: the options of
``embedding_model_params``, the per-relation Bernoulli thresholds (Wang et al. 2014, TransH) and the sorted keys of the known
triples.  The draw itself runs on the device (csrc/emg_sampler.hpp; contract: include/emgraph_hip.h, ``emg_sampler_bind``)."""
from __future__ import annotations

import numpy as np

SIDE_SAMPLINGS = ("uniform", "bernoulli")
DEFAULT_RETRIES = 4
KEYS = ("negative_side_sampling", "filter_negatives", "filter_negatives_retries", "negative_type_constraints")


def parse_params(params):
    """(side_sampling, filter, retries) of ``embedding_model_params``; anything out of range is a ValueError"""
    side = params.get("negative_side_sampling", "uniform")
    if not isinstance(side, str) or side not in SIDE_SAMPLINGS:
        raise ValueError("Invalid negative_side_sampling {!r}: expected 'uniform' or 'bernoulli'".format(side))
    flt = params.get("filter_negatives", False)
    if not isinstance(flt, (bool, np.bool_)):
        raise ValueError("Invalid filter_negatives {!r}: expected True or False".format(flt))
    retries = params.get("filter_negatives_retries", DEFAULT_RETRIES)
    if isinstance(retries, (bool, np.bool_)) or not isinstance(retries, (int, np.integer)) or not 1 <= int(retries) <= 255:
        raise ValueError("Invalid filter_negatives_retries {!r}: expected an int in 1..255".format(retries))
    type_constraints_param(params)
    return side, bool(flt), int(retries)


def type_constraints_param(params):
    """``embedding_model_params['negative_type_constraints']``: None (absent: untyped negatives), True (derive the pools from the
    training triples at fit) or a TypeConstraints (emgraph_amd/type_constraints.py); anything else is a ValueError.  Typed
    negatives (PyKEEN's pseudo-typed negatives; Krompass et al. 2015): the replacement of a corruption of relation p is drawn
    from the entities observed on that side of p instead of from all entities."""
    from .type_constraints import TypeConstraints
    if "negative_type_constraints" not in params:
        return None
    v = params["negative_type_constraints"]
    if v is True or isinstance(v, TypeConstraints):
        return v
    raise ValueError("Invalid negative_type_constraints {!r}: expected True or a TypeConstraints".format(v))


SHARED_NEGATIVES_MAX = 256   # the chunk sizes the shared-negatives kernels take (include/emgraph_hip.h, emg_shared_forward)
SHARED_REFUSES = ("sharding", "negative_side_sampling", "filter_negatives", "negative_type_constraints")


def shared_negatives_param(params):
    """``embedding_model_params['shared_negatives']``: None (absent: every positive draws its own negatives) or the chunk size C —
    chunks of C consecutive rows of a batch share one draw per (side, j), and every positive of a chunk is scored against all of
    them (DGL-KE's ``neg_chunk_size``, PyTorch-BigGraph's chunked uniform negatives).  Decided before any device
    work: anything but an int in [1, 256] is a ValueError; the key together with 'sharding', 'negative_side_sampling',
    'filter_negatives' or 'negative_type_constraints' (present, whatever the value) a NotImplementedError — the step is one GPU's,
    and per-row redraws contradict sharing."""
    if "shared_negatives" not in params:
        return None
    v = params["shared_negatives"]
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError("Invalid shared_negatives {!r}: expected an int in 1..{}".format(v, SHARED_NEGATIVES_MAX))
    if not 1 <= int(v) <= SHARED_NEGATIVES_MAX:
        raise ValueError("Invalid shared_negatives {}: expected an int in 1..{}".format(v, SHARED_NEGATIVES_MAX))
    for key in SHARED_REFUSES:
        if key in params and params[key] is not None:
            raise NotImplementedError("embedding_model_params['shared_negatives'] is not available together with "
                                      "embedding_model_params[{!r}]".format(key))
    return int(v)


ENTITY_SIDES = ("s", "o", "s+o", "s,o")
RELATION_SIDE = "p"
RELATION_SIDE_REFUSES = ("sharding", "shared_negatives", "negative_side_sampling", "filter_negatives", "negative_type_constraints")


def canonical_sides(sides):
    """The corruption sides of a training run in slot order: the entity sides in the order given, then 'p' (relation negatives,
    DESIGN.md A-28) wherever it stood in the list.  A str stands for a list of one.  ValueError: an unknown side, 'p' twice."""
    if isinstance(sides, str):
        sides = [sides]
    sides = list(sides)
    for s in sides:
        if s not in ENTITY_SIDES and s != RELATION_SIDE:
            raise ValueError("Invalid argument value {} for corruption side passed for evaluation.".format(s))
    if sides.count(RELATION_SIDE) > 1:
        raise ValueError("Invalid corruption sides {!r}: 'p' (relation negatives) may be listed at most once".format(sides))
    return [s for s in sides if s != RELATION_SIDE] + [RELATION_SIDE] * sides.count(RELATION_SIDE)


def check_relation_side(params):
    """What fit() refuses, before any device work, when 'p' is among the corruption sides: the key together with 'sharding',
    'shared_negatives', 'negative_side_sampling', 'filter_negatives' or 'negative_type_constraints' (present, whatever the value) is a
    NotImplementedError, each by name — relation negatives are one GPU's host-driven step with the ordinary draw
    ('negative_corruption_entities' keeps its meaning for the entity sides and does not touch the relation side)."""
    for key in RELATION_SIDE_REFUSES:
        if key in params and params[key] is not None:
            raise NotImplementedError("corrupt_sides with 'p' (relation negatives) is not available together with "
                                      "embedding_model_params[{!r}]".format(key))


BATCH_REGULARIZERS = ("batch_LP", "N3")
BATCH_REGULARIZER_REFUSES = ("sharding", "shared_negatives", "negative_side_sampling", "filter_negatives", "negative_type_constraints")
DEFAULT_BATCH_REGULARIZER_LAMBDA = 1e-5   # (the full-table LP's default)


def batch_regularizer_params(name, params, pair_rows=False, phase_relations=False):
    """The batch-local regulariser of ``regularizer=name`` ('batch_LP' | 'N3') and ``regularizer_params``, decided
    without a device: {'p': 1..3, 'lambda_ent', 'lambda_rel', 'modulus_ent', 'modulus_rel'}.
    'batch_LP': 'p' an int in 1..3 (default 3), 'lambda' a non-negative scalar or [lambda_ent, lambda_rel] (default 1e-5), 'modulus' a
    bool (default True) that counts only for models whose rows are [re | im] (``pair_rows``).  'N3' = 'batch_LP' with p = 3 and the
    modulus form: only 'lambda' is read, a 'p' other than 3 is a ValueError.  ``phase_relations`` (RotatE: relation rows are phases):
    a scalar 'lambda' applies to the entities alone, an explicit non-zero lambda_rel is a ValueError.  Anything else: ValueError."""
    if name not in BATCH_REGULARIZERS:
        raise ValueError("Unsupported regularizer: {}".format(name))
    params = params or {}
    p = params.get("p", 3)
    if isinstance(p, (bool, np.bool_)) or not isinstance(p, (int, np.integer)) or not 1 <= int(p) <= 3:
        raise ValueError("Invalid value for regularizer parameter p:{}. {!r} takes an int in 1..3".format(p, name))
    modulus = params.get("modulus", True)
    if name == "N3":
        if int(p) != 3:
            raise ValueError("regularizer 'N3' is the cube of the modulus: p = {} is not 3 (use 'batch_LP')".format(p))
        modulus = True
    elif not isinstance(modulus, (bool, np.bool_)):
        raise ValueError("Invalid value for regularizer parameter modulus:{!r}. Expected True or False".format(modulus))
    lam = params.get("lambda", DEFAULT_BATCH_REGULARIZER_LAMBDA)
    scalar = np.isscalar(lam)
    if scalar:
        lam = [lam, lam]
    elif not (isinstance(lam, (list, tuple)) and len(lam) == 2 and all(np.isscalar(v) for v in lam)):
        raise ValueError("Regularizer weight must be a scalar or a list with length equal to number of params passes")
    try:
        lam = [float(v) for v in lam]
    except (TypeError, ValueError):
        raise ValueError("Regularizer weight must be a number, got {!r}".format(params.get("lambda")))
    if not all(np.isfinite(v) and v >= 0.0 for v in lam):
        raise ValueError("Regularizer weight must be finite and non-negative, got {!r}".format(params.get("lambda")))
    if phase_relations:
        if not scalar and lam[1] != 0.0:
            raise ValueError("the relation rows of this model are phases and are not regularised: lambda_rel = {} must be 0 (a scalar "
                             "'lambda' applies to the entities alone)".format(lam[1]))
        lam[1] = 0.0
    modulus = bool(modulus) and bool(pair_rows)
    return {"p": int(p), "lambda_ent": lam[0], "lambda_rel": lam[1], "modulus_ent": modulus,
            "modulus_rel": modulus and not phase_relations}


def check_batch_regularizer(params, sides=()):
    """What fit() refuses, before any device work, under a batch-local regulariser: 'sharding', 'shared_negatives',
    'negative_side_sampling', 'filter_negatives' or 'negative_type_constraints' among ``embedding_model_params`` (present, whatever the
    value), and 'p' among the corruption ``sides`` — a NotImplementedError each, the key named: the step is one GPU's host-driven
    step with the ordinary draw."""
    for key in BATCH_REGULARIZER_REFUSES:
        if key in params and params[key] is not None:
            raise NotImplementedError("a batch regulariser ('batch_LP' / 'N3') is not available together with "
                                      "embedding_model_params[{!r}]".format(key))
    if RELATION_SIDE in (sides if not isinstance(sides, str) else [sides]):
        raise NotImplementedError("a batch regulariser ('batch_LP' / 'N3') is not available together with 'p' among the corruption "
                                  "sides (relation negatives)")


def asked(params):
    """one of the keys is present (whatever its value): what a sharded fit refuses"""
    return any(k in params for k in KEYS)


def keys_fit(n_ent, n_rel):
    """(s * n_rel + p) * n_ent + o fits 63 bits for every triple"""
    return int(n_ent) * int(n_ent) * int(n_rel) < (1 << 63)


def check_fit(params, sharding, n_ent, n_rel):
    """What fit() decides before any device work: (side_sampling, filter, retries), or the refusals — ValueError for a value out
    of range; NotImplementedError for one of the keys together with ``embedding_model_params['sharding']`` (``sharding``: 'k',
    'batch' or None; on any number of ranks) and for a filter whose keys would not fit.  ``negative_type_constraints``
    (``type_constraints_param`` returns it) is validated here too: a ValueError together with a ``negative_corruption_entities``
    other than 'all', or for constraints built for tables of another size."""
    side, flt, retries = parse_params(params)
    if sharding in ("k", "batch") and asked(params):
        raise NotImplementedError("negative_side_sampling / filter_negatives / negative_type_constraints train on one GPU; sharding "
                                  "{!r} does not carry them".format(sharding))
    tc = type_constraints_param(params)
    if tc is not None:
        if params.get("negative_corruption_entities", "all") != "all":
            raise ValueError("negative_type_constraints draw from the pools of the relations: not together with "
                             "negative_corruption_entities={!r}".format(params.get("negative_corruption_entities")))
        if tc is not True and (tc.n_ent != int(n_ent) or tc.n_rel != int(n_rel)):
            raise ValueError("negative_type_constraints were built for {} entities and {} relations, the training set has {} and "
                             "{}".format(tc.n_ent, tc.n_rel, n_ent, n_rel))
    if flt and not keys_fit(n_ent, n_rel):
        raise NotImplementedError("filter_negatives needs n_ent^2 * n_rel < 2^63 (the key of a triple): {} entities, {} "
                                  "relations".format(n_ent, n_rel))
    return side, flt, retries


def bernoulli_thresholds(X_idx, n_rel):
    """uint32 [n_rel]: keep_thr[p] = min(2^32 - 1, floor(|S_p| 2^32 / (|S_p| + |O_p|))), S_p / O_p the distinct subjects / objects
    of relation p in ``X_idx`` (int [n, 3]) — the subject is KEPT (the object replaced) with probability |S_p| / (|S_p| + |O_p|),
    i.e. replaced with tph / (tph + hpt).  A relation without triples gets 2^31 (a fair coin; never drawn)."""
    X = np.asarray(X_idx, dtype=np.int64).reshape(-1, 3)
    n_rel = int(n_rel)
    span = int(max(X[:, 0].max(initial=0), X[:, 2].max(initial=0))) + 1          # (pairs packed into one integer: 1-D unique passes)
    ps = np.unique(X[:, 1] * span + X[:, 0]) // span
    po = np.unique(X[:, 1] * span + X[:, 2]) // span
    n_s = np.bincount(ps, minlength=n_rel)[:n_rel]
    n_o = np.bincount(po, minlength=n_rel)[:n_rel]
    a, b = n_s.astype(np.uint64), n_o.astype(np.uint64)          # (counts < 2^31: a << 32 fits 64 bits, the division is exact)
    thr = np.minimum((a << np.uint64(32)) // np.maximum(a + b, np.uint64(1)), np.uint64((1 << 32) - 1))
    return np.where(a + b > 0, thr, np.uint64(1 << 31)).astype(np.uint32)


def known_triple_keys(X_idx, n_ent, n_rel):
    """int64 [m]: the ascending distinct keys (s * n_rel + p) * n_ent + o of the triples ``X_idx`` (below 2^63: ``keys_fit``)"""
    X = np.asarray(X_idx, dtype=np.int64).reshape(-1, 3)
    return np.unique((X[:, 0] * int(n_rel) + X[:, 1]) * int(n_ent) + X[:, 2])
