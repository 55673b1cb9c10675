"""EmbeddingModel and the four hot-path models — host-side mirror of emgraph/models/EmbeddingModel.py
(fit :1113-1492, predict :2101-2186, get_ranks :2046-2099, get_embeddings :455-488) and of
TransE.py / DistMult.py / ComplEx.py / HolE.py (which only contribute ``_fn`` and ``internal_k``).

Same constructor arguments, defaults (utils/constants.py) and error behaviour; the per-batch work is
done by libemgraph_hip.so through emgraph_amd.training.Trainer / emgraph_amd.evaluation.ranking.

Deliberate deviations from the reference's *literal* TF2-port behaviour, all in
favour of its intended (AmpliGraph-1.x) semantics: every batch is trained on exactly once (A-2);
optimizer state persists across batches (A-3); ranks are computed per test triple (A-1); both
'corrupt_side' and 'corrupt_sides' keys are honoured (A-5); large-graph host paging is not needed on a
288 GB GPU, so |E| > ENTITY_THRESHOLD neither pages nor forces SGD.
"""
from __future__ import annotations

import abc
import logging

import numpy as np
import torch

from .. import _lib as L
from .. import _switches
from .. import device as D
from .. import negative_sampling
from .. import parallel
from ..datasets import EmgraphBaseDatasetAdaptor
from ..evaluation.metrics import hits_at_n_score, mrr_score
from ..evaluation.protocol import _lookup, create_mappings_and_index, to_idx
from ..evaluation.ranking import FilterIndex, rank_triples_device
from ..training import Trainer, alloc_table, focuse_edge_weights, focuse_fill_and_mean

logger = logging.getLogger(__name__)

MODEL_REGISTRY = {}

# utils/constants.py
DEFAULT_EMBEDDING_SIZE = 100
DEFAULT_ETA = 2
DEFAULT_EPOCH = 100
DEFAULT_BATCH_COUNT = 100
DEFAULT_SEED = 0
DEFAULT_OPTIM = "adam"
DEFAULT_LR = 0.0005
DEFAULT_LOSS = "nll"
DEFAULT_REGULARIZER = None
DEFAULT_INITIALIZER = "glorot_uniform"
DEFAULT_VERBOSE = False
DEFAULT_NORM_TRANSE = 1
DEFAULT_CORRUPTION_ENTITIES = "all"
DEFAULT_CORRUPT_SIDE_TRAIN = ["s,o"]
DEFAULT_CORRUPT_SIDE_EVAL = "s,o"
DEFAULT_NORMALIZE_EMBEDDINGS = False
DEFAULT_BURN_IN_EARLY_STOPPING = 100
DEFAULT_CHECK_INTERVAL_EARLY_STOPPING = 10
DEFAULT_STOP_INTERVAL_EARLY_STOPPING = 3
DEFAULT_CRITERIA_EARLY_STOPPING = "mrr"
DEFAULT_RANK_COMPARE_STRATEGY = "worst"
# initializers/_initializer_constants.py
DEFAULT_UNIFORM_LOW, DEFAULT_UNIFORM_HIGH = -0.05, 0.05
DEFAULT_NORMAL_MEAN, DEFAULT_NORMAL_STD = 0, 0.05
DEFAULT_GLOROT_IS_UNIFORM = False

ENTITY_THRESHOLD = 5e5  # EmbeddingModel.py:37 (kept for API parity; no host paging here)

LOSSES = ("pairwise", "nll", "absolute_margin", "self_adversarial", "multiclass_nll")
OPTIMIZERS = ("adam", "adagrad", "sgd", "momentum", "adam_lazy")
INITIALIZERS = ("glorot_uniform", "normal", "uniform", "constant")


def set_entity_threshold(threshold):
    """EmbeddingModel.py:41-49 (API parity)."""
    global ENTITY_THRESHOLD
    ENTITY_THRESHOLD = threshold


def reset_entity_threshold():
    """EmbeddingModel.py:52-58 (API parity)."""
    global ENTITY_THRESHOLD
    ENTITY_THRESHOLD = 5e5


def register_model(name):
    def deco(cls):
        MODEL_REGISTRY[name] = cls
        cls.name = name
        return cls
    return deco


def _initial_table(kind, params, rnd, rows, cols, concept):
    """initializers/*.py numpy paths.  glorot_uniform follows the reference's TF path, which ALWAYS
    returns tf.initializers.GlorotUniform() whatever the 'uniform' flag says (glorot_uniform.py:59-74,
    SURVEY A-11): U(+-sqrt(6/(rows+cols))).  The draws themselves are parity-unpinned (TF RNG)."""
    if kind == "glorot_uniform":
        limit = np.sqrt(6 / (rows + cols))
        return rnd.uniform(-limit, limit, size=(rows, cols)).astype(np.float32)
    if kind == "normal":
        return rnd.normal(params.get("mean", DEFAULT_NORMAL_MEAN), params.get("std", DEFAULT_NORMAL_STD),
                          size=(rows, cols)).astype(np.float32)
    if kind == "uniform":
        return rnd.uniform(params.get("low", DEFAULT_UNIFORM_LOW), params.get("high", DEFAULT_UNIFORM_HIGH),
                           size=(rows, cols)).astype(np.float32)
    if kind == "constant":
        arr = np.asarray(params["entity" if concept == "e" else "relation"], dtype=np.float32)
        assert arr.shape == (rows, cols), "Invalid shape for {} initializer!".format(
            "entity" if concept == "e" else "relation")
        return arr
    raise ValueError("Unsupported initializer: {}".format(kind))


def _initial_table_device(kind, params, seed, rows, cols, concept, device):
    """the same initialisers drawn on the device (emg_init_table, Philox keyed by (seed, table)): no 1M x 400 float64
    array on the host.  Returns a float32 device tensor [rows, cols] (row stride padded to 16 bytes), or None for
    initialisers that have no device form ('constant')."""
    from ..training import alloc_table
    stream_id = 1 if concept == "e" else 2
    if kind == "glorot_uniform":
        limit = float(np.sqrt(6 / (rows + cols)))
        spec = ("uniform", -limit, limit)
    elif kind == "uniform":
        spec = ("uniform", params.get("low", DEFAULT_UNIFORM_LOW), params.get("high", DEFAULT_UNIFORM_HIGH))
    elif kind == "normal":
        spec = ("normal", params.get("mean", DEFAULT_NORMAL_MEAN), params.get("std", DEFAULT_NORMAL_STD))
    else:
        return None
    t = alloc_table(rows, cols, device)
    return D.init_table(t, cols, spec[0], spec[1], spec[2], seed, stream_id)


class EmbeddingModel(abc.ABC):  # noqa: B024
    """Abstract base of the embedding models (EmbeddingModel.py:96-336)."""

    name = "EmbeddingModel"
    _pair_rows = False          # entity rows are [re | im]: a batch regulariser takes the modulus form by default (A-29)
    _phase_relations = False    # relation rows are phases: no regulariser touches them

    def __init__(self, k=DEFAULT_EMBEDDING_SIZE, eta=DEFAULT_ETA, epochs=DEFAULT_EPOCH,
                 batches_count=DEFAULT_BATCH_COUNT, seed=DEFAULT_SEED, embedding_model_params={},
                 optimizer=DEFAULT_OPTIM, optimizer_params={"lr": DEFAULT_LR}, loss=DEFAULT_LOSS, loss_params={},
                 regularizer=DEFAULT_REGULARIZER, regularizer_params={}, initializer=DEFAULT_INITIALIZER,
                 initializer_params={"uniform": DEFAULT_GLOROT_IS_UNIFORM}, large_graphs=False,
                 verbose=DEFAULT_VERBOSE):
        if loss == "bce":  # EmbeddingModel.py:206-210: BCE is ConvE-only
            raise ValueError("Invalid Model - Loss combination. "
                             "ConvE model can be used with BCE loss only and vice versa.")
        self.all_params = {
            "k": k, "eta": eta, "epochs": epochs, "batches_count": batches_count, "seed": seed,
            "embedding_model_params": embedding_model_params, "optimizer": optimizer,
            "optimizer_params": optimizer_params, "loss": loss, "loss_params": loss_params,
            "regularizer": regularizer, "regularizer_params": regularizer_params, "initializer": initializer,
            "initializer_params": initializer_params, "verbose": verbose,
        }
        self.seed = seed
        self.loss_params = loss_params
        # a copy: the subclasses' default dictionaries are shared objects (EmbeddingModel.py has the same mutable defaults;
        # there a model that edits its params edits every later model's defaults)
        self.embedding_model_params = dict(embedding_model_params)
        self.k = k
        self.internal_k = k
        self.epochs = epochs
        self.eta = eta
        self.regularizer_params = regularizer_params
        self.batches_count = batches_count
        self.dealing_with_large_graphs = large_graphs
        if batches_count == 1:
            logger.warning("All triples will be processed in the same batch (batches_count=1). "
                           "When processing large graphs it is recommended to batch the input knowledge graph "
                           "instead.")
        if loss not in LOSSES:
            msg = "Unsupported loss function: {}".format(loss)
            logger.error(msg)
            raise ValueError(msg)
        self.loss = loss
        if regularizer is not None and regularizer != "LP" and regularizer not in negative_sampling.BATCH_REGULARIZERS:
            msg = "Unsupported regularizer: {}".format(regularizer)
            logger.error(msg)
            raise ValueError(msg)
        self.regularizer = regularizer
        # 'batch_LP' / 'N3' (not in the reference): the parameters are judged here, without a device
        self._batch_regularizer = (negative_sampling.batch_regularizer_params(regularizer, regularizer_params, self._pair_rows,
                                                                              self._phase_relations)
                                   if regularizer in negative_sampling.BATCH_REGULARIZERS else None)
        if optimizer not in OPTIMIZERS:
            msg = "Unsupported optimizer: {}".format(optimizer)
            logger.error(msg)
            raise ValueError(msg)
        self.optimizer = optimizer
        self.optimizer_params = optimizer_params
        self.verbose = verbose
        if initializer not in INITIALIZERS:
            msg = "Unsupported initializer: {}".format(initializer)
            logger.error(msg)
            raise ValueError(msg)
        self.initializer = initializer
        self.initializer_params = initializer_params
        self.trained_model_params = []
        self.is_fitted = False
        self.is_filtered = False
        self.eval_config = {}
        self.is_calibrated = False
        self.calibration_parameters = []
        self.ent_to_idx = {}
        self.rel_to_idx = {}
        self._dev = None  # (ent, rel) device tables of the trained parameters

    # ---- model-specific hooks ----
    def _model_id(self):
        raise NotImplementedError

    def _scale(self):
        return 1.0

    def _fn(self, e_s, e_p, e_o):
        """Score of already-gathered embedding rows [n, internal_k] — the reference's extension contract
        (EmbeddingModel.py:316-336; TransE.py:208-216, DistMult.py:201, ComplEx.py:288-298, HolE.py:189).
        Runs through the same HIP gather+score kernel as everything else (rows are staged as two small
        tables); fit/predict/evaluation never call it because their gathers are fused into the kernels."""
        D.require_gpu()
        dev = torch.device("cuda")
        rows = [torch.as_tensor(np.asarray(a, dtype=np.float32) if not isinstance(a, torch.Tensor) else a,
                                dtype=torch.float32, device=dev) for a in (e_s, e_p, e_o)]
        n, kk = rows[0].shape
        ent = alloc_table(2 * n, kk, dev)
        rel = alloc_table(n, kk, dev)
        ent[:n].copy_(rows[0])
        ent[n:].copy_(rows[2])
        rel.copy_(rows[1])
        ar = torch.arange(n, dtype=torch.int32, device=dev)
        spo = torch.stack([ar, ar, ar + n], dim=1).contiguous()
        return D.score_triples(self._model_id(), ent, rel, kk, self._scale(), spo).cpu().numpy()

    def _initial_relation_table(self, n_rel, dev, rnd=None):
        """the relation table fit() starts from: the model's initializer, drawn on the device, or — ``rnd`` given: the initializer has
        no device form ('constant') — on the host"""
        if rnd is not None:
            return _initial_table(self.initializer, self.initializer_params, rnd, n_rel, self.internal_k, "r")
        return _initial_table_device(self.initializer, self.initializer_params, self.seed, n_rel, self.internal_k, "r", dev)

    def _refuse_without_kernel(self, what):
        """raises NotImplementedError where the model has no kernel for ``what`` (RotatE); called before the device is asked for"""

    # ---- bookkeeping mirrored from the reference ----
    def get_hyperparameter_dict(self):
        return self.all_params

    def get_embedding_model_params(self, output_dict):
        output_dict["model_params"] = self.trained_model_params
        output_dict["large_graph"] = self.dealing_with_large_graphs
        output_dict["calibration_parameters"] = self.calibration_parameters

    def restore_model_params(self, in_dict):
        self.trained_model_params = [np.asarray(p, dtype=np.float32) for p in in_dict["model_params"]]
        self.calibration_parameters = in_dict.get("calibration_parameters", [])
        self.dealing_with_large_graphs = in_dict.get("large_graph", False)
        self._dev = None

    def get_embeddings(self, entities, embedding_type="entity"):
        """EmbeddingModel.py:455-488."""
        if not self.is_fitted:
            msg = "Model has not been fitted."
            logger.error(msg)
            raise RuntimeError(msg)
        if embedding_type == "entity":
            emb_list, lookup_dict = self.trained_model_params[0], self.ent_to_idx
        elif embedding_type == "relation":
            emb_list, lookup_dict = self.trained_model_params[1], self.rel_to_idx
        else:
            msg = "Invalid entity type: {}".format(embedding_type)
            logger.error(msg)
            raise ValueError(msg)
        # one sorted-key search for the whole array (the reference maps label by label: np.vectorize(dict.get)); a label the
        # model was not fitted on fails like the reference's None index does
        labels = np.asarray(entities)
        idxs, known = _lookup(labels.reshape(-1), lookup_dict)
        if not known.all():
            raise IndexError("get_embeddings: label(s) not seen in training: %r" % (labels.reshape(-1)[~known][:5].tolist(),))
        return emb_list[idxs.reshape(labels.shape)]

    def is_fitted_on(self, X):
        """EmbeddingModel.py:2188-2210."""
        if not self.is_fitted:
            msg = "Model has not been fitted."
            logger.error(msg)
            raise RuntimeError(msg)
        unique_ent = np.unique(np.concatenate((X[:, 0], X[:, 2])))
        unique_rel = np.unique(X[:, 1])
        return len(unique_ent) == len(self.ent_to_idx) and len(unique_rel) == len(self.rel_to_idx)

    # ---- training ----
    def _corrupt_sides(self):
        p = self.embedding_model_params
        sides = p.get("corrupt_side", p.get("corrupt_sides", DEFAULT_CORRUPT_SIDE_TRAIN))  # SURVEY A-5
        if not isinstance(sides, list):
            sides = [sides]
        # 'p' (relation negatives; not in the reference) at most once: the entity sides in the order given, then 'p'
        return negative_sampling.canonical_sides(sides)

    def _relation_side(self):
        """'p' is among the corruption sides (relation negatives); the list itself is judged by _corrupt_sides"""
        p = self.embedding_model_params
        sides = p.get("corrupt_side", p.get("corrupt_sides", DEFAULT_CORRUPT_SIDE_TRAIN))
        return negative_sampling.RELATION_SIDE in (sides if isinstance(sides, list) else [sides])

    def _negative_pool(self, X_idx, batch_size):
        """negative_corruption_entities (EmbeddingModel.py:731-783): 'all' | 'batch' | list of labels | int.
        Returns (n_choices or None, fixed entities_list tensor or None, per-batch lists or None)."""
        nce = self.embedding_model_params.get("negative_corruption_entities", DEFAULT_CORRUPTION_ENTITIES)
        if isinstance(nce, str) and nce == "all":
            return len(self.ent_to_idx), None, None
        if isinstance(nce, str) and nce == "batch":
            from ..evaluation.protocol import batch_entities
            lists = []
            for i in range(self.batches_count):
                xb = X_idx[i * batch_size:(i + 1) * batch_size]
                lists.append(torch.from_numpy(batch_entities(xb)).cuda() if len(xb) else None)
            return None, None, lists
        if isinstance(nce, list):
            wanted = set(nce)
            ids = np.asarray([idx for uri, idx in self.ent_to_idx.items() if uri in wanted], dtype=np.int32)
            return len(ids), torch.from_numpy(ids).cuda(), None
        if isinstance(nce, (int, np.integer)) and not isinstance(nce, bool):
            return int(nce), None, None
        raise ValueError("Invalid negative_corruption_entities: {}".format(nce))

    def _link(self):
        """embedding_model_params['non_linearity'] (EmbeddingModel.py:679-690): 'linear' | 'tanh' | 'sigmoid' | 'softplus'"""
        link = self.embedding_model_params.get("non_linearity", "linear")
        if link not in L.LINK_IDS:
            raise ValueError("Invalid non-linearity")
        return link

    def _rank_through_link(self):
        """embedding_model_params['rank_through_link'] (not in the reference's parameter list; default False): True lets
        get_ranks / evaluate_performance / early stopping rank a model with a non-linear ``non_linearity`` THROUGH the link, as
        the reference does (EmbeddingModel.py:1868-1879).  No effect under the linear link.  Anything but a bool: ValueError."""
        v = self.embedding_model_params.get("rank_through_link", False)
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError("rank_through_link must be True or False, got {!r}".format(v))
        return bool(v)

    def _refuse_ranking_under_link(self, what, always=False):
        """Ranks compare int32(score * 1e5) (EmbeddingModel.py:2010-2014): through a non-linear link that makes new ties, and the
        prefilters' thresholds are derived for the raw score — ranking through the link is opt-in
        (embedding_model_params['rank_through_link'], DESIGN.md 4.2 "Ranking through a link").  ``always``: callers whose kernels
        do not carry the link (discover_facts' grid ranking) refuse with or without the key."""
        through = self._rank_through_link()
        if self._link() != "linear" and (always or not through):
            raise NotImplementedError(
                "{} under non_linearity={!r} is not available{}: ranking is built for the linear score".format(
                    what, self._link(), " (with or without rank_through_link)" if always else
                    "; set embedding_model_params['rank_through_link'] = True to rank through the link"))

    def _rank_link_id(self):
        """the L.LINK_* id the ranking calls compare through (callers have passed _refuse_ranking_under_link)"""
        return L.LINK_IDS[self._link()]

    def fit(self, X, early_stopping=False, early_stopping_params={}, focusE_numeric_edge_values=None,
            tensorboard_logs_path=None):
        """Train the model (EmbeddingModel.py:1113-1492).  ``X``: ndarray [n,3] of labels, or a dataset adapter.
        ``focusE_numeric_edge_values`` [n] or [n, c] (NaN = unknown): FocusE (:679-722, 801-816, 1168-1228) — every
        triple's scores are weighted by its normalised edge value, blended towards 1 by the structure weight of the epoch
        (embedding_model_params 'stop_epoch', 'structural_wt', 'normalize_numeric_values'); an adapter that carries
        edge values for its train split turns it on as well (its values are used as they are — the reference normalises only
        what fit() itself wraps — and the ``focusE_numeric_edge_values`` argument is then ignored, with a warning).
        FocusE and non-linear links train on one GPU: with ``embedding_model_params['sharding']`` set they are refused, on any
        number of ranks (a configuration gives the same answer on every box).
        Negative sampling beyond the reference's fair coin and uniform replacement (``embedding_model_params``; not in the
        reference — OpenKE ``bern``, PyKEEN ``BernoulliNegativeSampler`` / ``filtered=True``; DESIGN.md 4.1 "Negative sampling"):
        ``'negative_side_sampling'``: ``'uniform'`` (default) | ``'bernoulli'`` — for the sides 's,o' / 's+o' the subject of a
        triple of relation p is replaced with probability tph / (tph + hpt) (Wang et al. 2014), from the distinct subjects and
        objects of p in X; ``'filter_negatives'``: ``False`` (default) | ``True`` — a corruption that is itself a triple of X is
        redrawn, up to ``'filter_negatives_retries'`` (1..255, default 4) times, the last draw kept.  Any other value is a
        ``ValueError``; either key with ``'sharding'`` set, and a filter with n_ent^2 * n_rel >= 2^63, a ``NotImplementedError``.
        ``calibrate()``, evaluation and early stopping draw as ever.  After ``fit()``, ``negative_sampling_stats`` is ALWAYS set:
        {'rows': corruption rows drawn, 'redrawn': rows whose final draw is a redraw, 'known_left': rows whose final candidate
        is still a triple of X} — counted on the device and read once; with both options off: the row count and zeros.
        ``'negative_type_constraints'``: ``True`` (the pools are the subjects / objects observed per relation in X) or a
        ``TypeConstraints`` — TYPED negatives (PyKEEN's pseudo-typed negatives): the replacement of a corruption
        comes from the domain (subject replaced) or range (object replaced) pool of the triple's relation, a side without a
        constraint from all entities; composes with the two options above (redraws come from the same pool).  Refused like
        them with ``'sharding'``; a ``ValueError`` for any other value and together with a ``'negative_corruption_entities'``
        other than 'all'.  ``negative_sampling_stats`` then also holds 'typed_rows': the rows drawn from a non-empty pool.
        ``'shared_negatives'``: C, an int in 1..256 — SHARED negatives (DGL-KE ``neg_chunk_size``, PyTorch-BigGraph's chunked
        uniform negatives; DESIGN.md A-26, 4.1 "Shared negatives"): every batch is cut into chunks of C consecutive triples, a
        chunk draws ONE replacement (and, for 's,o', one coin) per (side, j) and every triple of the chunk is scored against all
        eta of them — the ordinary step with codes[(sd eta + j) B + i] = chunk_codes[(sd eta + j) G + i // C].  Each triple still
        sees eta negatives per side; the step gathers and writes 2 + eta sides / C entity rows per triple instead of 2 + eta sides.
        Any other value is a ``ValueError``; the key together with ``'sharding'``, ``'negative_side_sampling'``,
        ``'filter_negatives'`` or ``'negative_type_constraints'`` a ``NotImplementedError`` — both decided before any device
        work.  ``negative_sampling_stats['rows']`` then counts the draws made: G eta sides per batch.
        ``'corrupt_sides'`` / ``'corrupt_side'`` may contain ``'p'``, at most once — RELATION negatives (PyKEEN
        ``corruption_scheme=('h','r','t')``, LibKGE ``num_samples.p``, OpenKE ``neg_rel``; DESIGN.md A-28, 4.1 "Relation negatives"):
        eta more negatives per positive (s, p, o) that keep s and o and replace p by one of the OTHER relations, uniformly (never the
        positive itself).  Alone (``'p'``) or beside entity sides (``['s,o', 'p']``); the slots are the entity sides in the order
        given, then 'p'.  ``'negative_corruption_entities'`` does not touch the relation side.  ``'p'`` twice and a training set of
        fewer than two relations are a ``ValueError``; ``'p'`` together with ``'sharding'`` or a multi-GPU job, ``'shared_negatives'``,
        ``'negative_side_sampling'``, ``'filter_negatives'``, ``'negative_type_constraints'``, and TransE ``norm = inf`` a
        ``NotImplementedError``.
        The constructor's ``regularizer`` takes, beside the reference's ``'LP'`` (the full tables), ``'batch_LP'`` and ``'N3'`` — the
        BATCH-LOCAL regulariser (LibKGE ``regularize_weighted``, PyKEEN ``LpRegularizer``, Lacroix et al. 2018; DESIGN.md A-29, 4.1
        "Batch regulariser"): R = sum_i [lambda_ent (N(E[s_i]) + N(E[o_i])) + lambda_rel N(R[p_i])] over the positives of a batch,
        every occurrence counted, a sum (LibKGE's lambda is lambda / B here), part of the reported loss.  ``regularizer_params``:
        ``'p'`` (1..3, default 3), ``'lambda'`` (a scalar or [lambda_ent, lambda_rel], default 1e-5), ``'modulus'`` (default True: for
        rows [re | im] — ComplEx, HolE, RotatE — N takes the complex modulus per coordinate; ignored for the other models); ``'N3'``
        is p = 3 on the modulus.  RotatE's relation rows (phases) are not regularised.  Together with ``'sharding'`` or a multi-GPU
        job, ``'shared_negatives'``, ``'p'`` among the corruption sides, ``'negative_side_sampling'``, ``'filter_negatives'`` or
        ``'negative_type_constraints'`` a ``NotImplementedError``."""
        self._refuse_without_kernel("fit")
        shared = negative_sampling.shared_negatives_param(self.embedding_model_params)
        if shared is not None and self._model_id() == L.TRANSE_P and np.isinf(self._scale()):
            raise NotImplementedError("embedding_model_params['shared_negatives'] is not available with TransE of norm inf (the "
                                      "gradient of a maximum shared by ties has no form in the shared-negatives kernels)")
        relation_side = self._relation_side()
        if relation_side:   # relation negatives (A-28): every refusal by name, before any device work
            negative_sampling.check_relation_side(self.embedding_model_params)
            if self._model_id() == L.TRANSE_P and np.isinf(self._scale()):
                raise NotImplementedError("corrupt_sides with 'p' (relation negatives) is not available with TransE of norm inf (the "
                                          "gradient of a maximum shared by ties has no form in the relation-negatives kernels)")
        if self._batch_regularizer is not None:   # batch-local regulariser (A-29): every refusal by name, before any device work
            p_ = self.embedding_model_params
            sides_ = p_.get("corrupt_side", p_.get("corrupt_sides", DEFAULT_CORRUPT_SIDE_TRAIN))
            negative_sampling.check_batch_regularizer(p_, sides_)
            if parallel.rank_world()[1] > 1:
                raise NotImplementedError("a batch regulariser ('batch_LP' / 'N3') trains on one GPU: not available in a multi-GPU job "
                                          "(embedding_model_params['sharding'] or several ranks)")
        D.require_gpu()
        link = self._link()
        if early_stopping:
            self._refuse_ranking_under_link("early stopping")
        edge_w = None
        # EmbeddingModel.py:1218-1248: an ndarray is wrapped in a NumpyDatasetAdapter; an adapter is used as it is
        if isinstance(X, np.ndarray):
            if X.ndim != 2 or X.shape[1] != 3:
                msg = "Invalid size for input X. Expected (n,3):  got {}".format(X.shape)
                logger.error(msg)
                raise ValueError(msg)
            handle = None
            if focusE_numeric_edge_values is not None:
                edge_w = focuse_edge_weights(X[:, 1], focusE_numeric_edge_values,
                                             normalize=self.embedding_model_params.get("normalize_numeric_values", True),
                                             seed=self.seed)
        elif isinstance(X, EmgraphBaseDatasetAdaptor):
            handle = X
            if focusE_numeric_edge_values is not None:   # (the reference drops the argument here without a word)
                logger.warning("focusE_numeric_edge_values is ignored when X is a dataset adapter: hand the values to the "
                               "adapter's set_data()")
        else:
            msg = "Invalid type for input X. Expected ndarray/EmgraphDataset object, got {}".format(type(X))
            logger.error(msg)
            raise ValueError(msg)
        if handle is None:
            self.rel_to_idx, self.ent_to_idx, X_idx = create_mappings_and_index(X)
        else:
            # the adapter owns mapping and batching (abstract_dataset_adapter.py): ids come from ITS dictionaries and
            # the training set is the concatenation of its batches, which stay contiguous slices of the resident copy
            self.rel_to_idx, self.ent_to_idx = handle.generate_mappings()
            handle.map_data()
            batches = [b if isinstance(b, (list, tuple)) else [b] for b in handle.get_next_batch(self.batches_count, "train")]
            parts = [np.asarray(b[0], dtype=np.int32).reshape(-1, 3) for b in batches]
            X_idx = np.concatenate(parts, axis=0) if parts else np.zeros((0, 3), np.int32)
            if batches and all(len(b) > 1 for b in batches):
                # the adapter hands edge values out with every batch (numpy_adapter.py:105-112): used as they are — the reference
                # normalises only what fit() itself wraps — unknown ones drawn, rows averaged (EmbeddingModel.py:1099-1108)
                vals = np.concatenate([np.asarray(b[1], dtype=np.float64).reshape(len(p_), -1) for b, p_ in zip(batches, parts)], axis=0)
                edge_w = focuse_fill_and_mean(vals, seed=self.seed)
            if X_idx.shape[0] != handle.get_size("train"):
                raise ValueError("the adapter's batches do not add up to get_size('train')")
        n = X_idx.shape[0]
        batch_size = int(np.ceil(n / self.batches_count))  # EmbeddingModel.py:1297-1301
        self.batch_size = batch_size
        rnd = np.random.RandomState(self.seed)  # refit -> same seed -> same run (EmbeddingModel.py:1286-1290)
        n_ent, n_rel = len(self.ent_to_idx), len(self.rel_to_idx)
        # drawn on the device where the initialiser has a device form (a pure function of (seed, table, shape): the same
        # table for any number of GPUs); 'constant' comes from the caller's arrays
        dev = torch.device("cuda")
        ent0 = _initial_table_device(self.initializer, self.initializer_params, self.seed, n_ent, self.internal_k, "e", dev)
        rel0 = self._initial_relation_table(n_rel, dev) if ent0 is not None else None
        if ent0 is None:
            ent0 = _initial_table(self.initializer, self.initializer_params, rnd, n_ent, self.internal_k, "e")
            rel0 = self._initial_relation_table(n_rel, dev, rnd)
        normalize = self.embedding_model_params.get("normalize_ent_emb", DEFAULT_NORMALIZE_EMBEDDINGS)
        rank, world = parallel.rank_world()
        # multi-GPU plan (one process per GPU): "k" = column slabs + all-reduce of partial scores (default);
        # "batch" = replicated tables, batch split over the ranks, sparse gradient-row exchange (parallel.py)
        sharding = self.embedding_model_params.get("sharding", _switches.get("EMG_SHARDING")) if world > 1 else None
        if sharding not in (None, "k", "batch"):
            raise ValueError("Invalid sharding {!r}: expected 'k' or 'batch'".format(sharding))
        if relation_side and (sharding or world > 1):   # (a sharding taken from the environment, or a job of several ranks)
            raise NotImplementedError("corrupt_sides with 'p' (relation negatives) trains on one GPU: not available with sharding "
                                      "{!r} / a multi-GPU job of {} ranks".format(sharding, world))
        if relation_side and n_rel < 2:
            raise ValueError("corrupt_sides with 'p' (relation negatives) needs at least two relations, the training set has "
                             "{}".format(n_rel))
        if shared is not None and sharding:   # (a sharding taken from the environment: the key itself was refused above)
            raise NotImplementedError("embedding_model_params['shared_negatives'] is not available together with sharding "
                                      "{!r}".format(sharding))
        self._sharded = sharding == "k"
        k_local = self.internal_k
        if self._sharded:
            # one process per GPU: this rank trains a COLUMN slab of both tables (parallel.py)
            if world > self.k:
                raise ValueError("k-sharded training needs k >= number of ranks (k={}, ranks={})".format(self.k, world))
            if normalize:
                raise NotImplementedError("normalize_ent_emb needs full rows; not available with k-sharded training")
        # (refused wherever a sharded fit is ASKED for, not only where more than one rank is running: the same answer on any box)
        asked = sharding or self.embedding_model_params.get("sharding")
        if asked in ("k", "batch") and (edge_w is not None or link != "linear"):
            raise NotImplementedError("FocusE edge values and non-linear score links train on one GPU; sharding {!r} does not carry "
                                      "them".format(asked))
        # negative sampling beyond the reference's (emgraph_amd/negative_sampling.py): validated whatever the values, refused with
        # sharding wherever one of the keys is present, built once per fit from the whole training set
        side_sampling, filter_neg, retries = negative_sampling.check_fit(self.embedding_model_params, asked, n_ent, n_rel)
        sampler = None
        typed = negative_sampling.type_constraints_param(self.embedding_model_params)
        if typed is True:   # the observed domains and ranges of the training triples
            from ..type_constraints import TypeConstraints
            typed = TypeConstraints.from_triples(X_idx, (n_ent, n_rel), from_idx=True)
        if side_sampling == "bernoulli" or filter_neg or typed is not None:
            sampler = {"keep_thr": negative_sampling.bernoulli_thresholds(X_idx, n_rel) if side_sampling == "bernoulli" else None,
                       "known_keys": negative_sampling.known_triple_keys(X_idx, n_ent, n_rel) if filter_neg else None,
                       "retries": retries, "type_constraints": typed}
        if self._sharded:
            cplx = self.internal_k != self.k
            ent0 = parallel.shard_columns(ent0, rank, world, cplx)
            rel0 = parallel.shard_columns(rel0, rank, world, cplx)
            k_local = ent0.shape[1]
        tr = Trainer(self._model_id(), k_local, self._scale(), ent0, rel0, self.eta, loss=self.loss,
                     loss_params=self.loss_params, optimizer=self.optimizer, optimizer_params=self.optimizer_params,
                     corrupt_sides=self._corrupt_sides(), batches_count=self.batches_count, seed=self.seed,
                     regularizer=self.regularizer, regularizer_params=self.regularizer_params,
                     normalize_ent_emb=normalize, sharded=sharding or False,
                     shard_state=bool(self.embedding_model_params.get("shard_state", False)) and sharding == "batch",
                     link=link, focuse_params=self.embedding_model_params, negative_sampler=sampler,
                     **({"shared_negatives": shared} if shared is not None else {}))
        tr.set_training_set(X_idx, batch_size, edge_w=edge_w)
        n_choices, fixed_list, batch_lists = self._negative_pool(X_idx, batch_size)
        if normalize:  # EmbeddingModel.py:1371-1380: both tables clipped once before the loop
            D.clip_rows(tr.rel, self.internal_k, 1.0)
            D.clip_rows(tr.ent, self.internal_k, 1.0)
        self.early_stopping_params = early_stopping_params
        es = self._initialize_early_stopping() if early_stopping else None
        # reported average: sum(losses) / (batch_size * batches_count), batch_size *= eta when the loss
        # tiles the positives (EmbeddingModel.py:1343-1344,1456)
        denom = batch_size * self.batches_count
        if self.loss in ("pairwise", "nll", "absolute_margin"):
            denom *= self.eta
        try:
            from tqdm import tqdm
            epochs_iter = tqdm(range(1, self.epochs + 1), disable=(not self.verbose), unit="epoch")
        except ImportError:  # pragma: no cover
            epochs_iter = range(1, self.epochs + 1)
        self._trainer = tr
        self.epoch_losses = []   # sum of the batch losses of each epoch (what the progress message averages)

        def batch_args(epoch, batch):
            """(start, B, epoch, batch, n_choices, entities_list) of a batch, or None past the end"""
            epoch, batch = epoch + (batch - 1) // self.batches_count, (batch - 1) % self.batches_count + 1
            if epoch > self.epochs:
                return None
            start = (batch - 1) * batch_size
            B = max(0, min(batch_size, n - start))  # last batch may be short / empty (numpy_adapter.py:105-112)
            if batch_lists is not None:
                elist = batch_lists[batch - 1]
                return (start, B, epoch, batch, elist.numel() if elist is not None else 0, elist)
            return (start, B, epoch, batch, n_choices, fixed_list)

        for epoch in epochs_iter:
            tr.run_batches([batch_args(epoch, batch) for batch in range(1, self.batches_count + 1)])
            loss_epoch = tr.read_loss()
            self.epoch_losses.append(loss_epoch)
            # EmbeddingModel.py:1422-1427 (per epoch here).  The reference's loss is a float32 tensor: a loss beyond float32's range IS inf
            # there; the device accumulates the epoch in a double, which would let such a run pass (seed 96078 of the round-6 soak)
            with np.errstate(over="ignore"):
                loss32 = np.float32(loss_epoch)
            if np.isnan(loss32) or np.isinf(loss32):
                msg = "Loss is {}. Please change the hyperparameters.".format(loss32)
                logger.error(msg)
                raise ValueError(msg)
            if self.verbose:
                msg = "Average {} Loss: {:10f}".format(self.name, loss_epoch / denom)
                if es is not None and es["best"] is not None:
                    msg += " — Best validation ({}): {:5f}".format(es["criteria"], es["best"])
                logger.debug(msg)
                if hasattr(epochs_iter, "set_description"):
                    epochs_iter.set_description(msg)
            if es is not None and self._perform_early_stopping_test(epoch, es, tr):
                self.negative_sampling_stats = tr.negative_sampling_stats()
                self.is_fitted = True
                return
        self.negative_sampling_stats = tr.negative_sampling_stats()
        self._save_trained_params(tr, live=True)
        self.is_fitted = True

    def _save_trained_params(self, tr, live=False):
        """Snapshot the tables into ``trained_model_params`` (EmbeddingModel.py:385-401).  ``live=True`` only for
        the final save at the end of fit(): inference may then read the trainer's tables directly.  A snapshot
        taken by early stopping must NOT alias them — training continues in place for ``stop_interval`` more
        checks, and predict()/get_ranks() have to use the best snapshot (the reference always infers from
        trained_model_params, :403-453) — so the device copy is dropped and re-uploaded lazily."""
        if getattr(self, "_sharded", False):
            cplx = self.internal_k != self.k
            ent = parallel.unshard_columns(parallel.gather_slabs(tr.ent), self.k, cplx)
            rel = parallel.unshard_columns(parallel.gather_slabs(tr.rel), self.k, cplx)
            self.trained_model_params = [ent, rel]
            self._dev = None  # full tables are uploaded lazily for predict / evaluation
            return
        ent, rel = tr.tables_numpy()
        self.trained_model_params = [ent, rel]
        self._dev = (tr.ent, tr.rel) if live else None

    def _eval_tables(self, tr):
        """full-width device tables of the CURRENT training state (early stopping)"""
        if not getattr(self, "_sharded", False):
            tr.materialize()   # (deferred dense decay: every row up to date before it is read)
            return tr.ent, tr.rel
        cplx = self.internal_k != self.k
        ent = parallel.unshard_columns(parallel.gather_slabs(tr.ent), self.k, cplx)
        rel = parallel.unshard_columns(parallel.gather_slabs(tr.rel), self.k, cplx)
        dev = torch.device("cuda")
        return alloc_table(ent.shape[0], ent.shape[1], dev, init=ent), alloc_table(rel.shape[0], rel.shape[1], dev, init=rel)

    # ---- early stopping (EmbeddingModel.py:824-1020) ----
    def _initialize_early_stopping(self):
        p = self.early_stopping_params
        try:
            x_valid = p["x_valid"]
        except KeyError:
            msg = "x_valid must be passed for early fitting."
            logger.error(msg)
            raise KeyError(msg)
        if isinstance(x_valid, EmgraphBaseDatasetAdaptor):   # EmbeddingModel.py:868-880: validation data held by an adapter
            if not x_valid.data_exists("valid"):
                msg = "Dataset `valid` has not been set in the DatasetAdapter."
                logger.error(msg)
                raise ValueError(msg)
            x_valid.use_mappings(self.rel_to_idx, self.ent_to_idx)
            x_valid.map_data()
            x_valid = np.concatenate([np.asarray(b[0]) for b in x_valid.get_next_batch(1, "valid")], axis=0)
            p = dict(p, x_valid=None)
            mapped_valid = x_valid
        else:
            mapped_valid = None
        if mapped_valid is None and not isinstance(x_valid, np.ndarray):
            msg = "Invalid type for input X. Expected ndarray/EmgraphDataset object, got {}".format(type(x_valid))
            logger.error(msg)
            raise ValueError(msg)
        if x_valid.ndim <= 1 or np.shape(x_valid)[1] != 3:
            msg = "Invalid size for input x_valid. Expected (n,3):  got {}".format(np.shape(x_valid))
            logger.error(msg)
            raise ValueError(msg)
        criteria = p.get("criteria", DEFAULT_CRITERIA_EARLY_STOPPING)
        if criteria not in ["hits10", "hits1", "hits3", "mrr"]:
            msg = "Unsupported early stopping criteria."
            logger.error(msg)
            raise ValueError(msg)
        ce = p.get("corruption_entities", DEFAULT_CORRUPTION_ENTITIES)
        subset = None
        if isinstance(ce, list):
            wanted = set(ce)
            subset = np.asarray([idx for uri, idx in self.ent_to_idx.items() if uri in wanted])
        cands = p.get("candidates")
        if cands is not None:   # the check ranks against K drawn candidates per triple and side (the same lists at every check)
            if isinstance(cands, bool) or not isinstance(cands, (int, np.integer)):
                raise ValueError("early_stopping_params['candidates'] must be an int K (the lists are drawn), got {!r}".format(cands))
            if cands < 1:
                raise ValueError("early_stopping_params['candidates'] must be at least 1, got %d" % cands)
            if subset is not None or not (isinstance(ce, str) and ce == "all"):
                raise ValueError("early_stopping_params['candidates'] and 'corruption_entities' both name the candidates: "
                                 "pass one of them")
            cands = int(cands)
        findex = None
        if "x_filter" in p:
            x_filter = p["x_filter"]
            if x_filter.ndim <= 1 or np.shape(x_filter)[1] != 3:
                msg = "Invalid size for input x_valid. Expected (n,3):  got {}".format(np.shape(x_filter))
                logger.error(msg)
                raise ValueError(msg)
            findex = FilterIndex(to_idx(x_filter, ent_to_idx=self.ent_to_idx, rel_to_idx=self.rel_to_idx))
        return {"x_valid": (mapped_valid if mapped_valid is not None else
                            to_idx(x_valid, ent_to_idx=self.ent_to_idx, rel_to_idx=self.rel_to_idx)),
                "criteria": criteria, "subset": subset, "filter": findex,
                "corrupt_side": p.get("corrupt_side", DEFAULT_CORRUPT_SIDE_EVAL),
                "candidates": cands, "candidates_seed": int(p.get("candidates_seed", 0)),
                "best": None, "first": None, "counter": 0, "epoch": None}

    def _perform_early_stopping_test(self, epoch, es, tr):
        p = self.early_stopping_params
        if not (epoch >= p.get("burn_in", DEFAULT_BURN_IN_EARLY_STOPPING)
                and epoch % p.get("check_interval", DEFAULT_CHECK_INTERVAL_EARLY_STOPPING) == 0):
            return False
        ent_f, rel_f = self._eval_tables(tr)
        ranks = rank_triples_device(self._model_id(), ent_f, rel_f, self.internal_k, self._scale(), es["x_valid"],
                                    es["corrupt_side"], DEFAULT_RANK_COMPARE_STRATEGY, filter_triples=es["filter"],
                                    entities_subset=es["subset"],
                                    shard=parallel.rank_world() if parallel.is_active() else None,
                                    precision=self._eval_precision(), link=self._rank_link_id(),
                                    candidates=es["candidates"], candidates_seed=es["candidates_seed"])
        crit = es["criteria"]
        cur = mrr_score(ranks) if crit == "mrr" else hits_at_n_score(ranks, int(crit[4:]))
        if es["best"] is None:
            es["best"] = es["first"] = cur
        elif es["best"] >= cur:
            es["counter"] += 1
            if es["counter"] == p.get("stop_interval", DEFAULT_STOP_INTERVAL_EARLY_STOPPING):
                if es["best"] == es["first"]:
                    self._save_trained_params(tr)
                if self.verbose:
                    logger.info("Early stopping at epoch:{}".format(epoch))
                    logger.info("Best {}: {:10f}".format(crit, es["best"]))
                self.early_stopping_epoch = epoch
                return True
        else:
            es["best"] = cur
            es["counter"] = 0
            self._save_trained_params(tr)
        return False

    # ---- inference ----
    def _device_tables(self):
        if self._dev is None:
            D.require_gpu()
            ent, rel = self.trained_model_params
            self._dev = (alloc_table(ent.shape[0], ent.shape[1], torch.device("cuda"), init=ent),
                         alloc_table(rel.shape[0], rel.shape[1], torch.device("cuda"), init=rel))
        return self._dev

    def predict(self, X, from_idx=False, chunk=1 << 22, sharded=False):
        """Scores of the triples X (EmbeddingModel.py:2101-2186).

        ``sharded=True`` (multi-GPU, one process per GPU): a COLLECTIVE — every rank must call it with the same X; rank r
        scores the r-th contiguous range of the list and the ranges are summed into place.  The default is rank-local
        (every rank scores everything it is given), so `if rank == 0: model.predict(...)` and models restored in one
        process of a distributed job work as on a single GPU."""
        if not self.is_fitted:
            msg = "Model has not been fitted."
            logger.error(msg)
            raise RuntimeError(msg)
        if sharded:
            self._refuse_without_kernel("predict(sharded=True)")
        link = self._link()
        if type(X) is not np.ndarray:
            X = np.array(X)
        if X.ndim == 1:
            X = X[np.newaxis, :]
        if not from_idx:
            X = to_idx(X, ent_to_idx=self.ent_to_idx, rel_to_idx=self.rel_to_idx)
        X = np.ascontiguousarray(X, dtype=np.int32)
        ent, rel = self._device_tables()
        out = np.zeros(X.shape[0], dtype=np.float32)
        # multi-GPU (one process per GPU, tables replicated): rank r scores the r-th contiguous range of the triple
        # list and the ranges are summed into place (predict shards trivially, no data-path exchange)
        rank, world = parallel.rank_world() if sharded else (0, 1)
        r0, r1 = parallel.entity_range(X.shape[0], rank, world)
        for c0 in range(r0, r1, chunk):  # SURVEY A-17: chunk instead of one giant gather
            c1 = min(c0 + chunk, r1)
            xt = torch.from_numpy(X[c0:c1]).cuda()
            sc = D.score_triples(self._model_id(), ent, rel, self.internal_k, self._scale(), xt)
            # EmbeddingModel.py:2135-2145: the link on the scores (the FocusE weights are training's alone)
            if link == "tanh":
                sc = torch.tanh(sc)
            elif link == "sigmoid":
                sc = torch.sigmoid(sc)
            elif link == "softplus":
                sc = torch.log(1 + 9999 * torch.exp(sc))   # custom_softplus, :90-96
            out[c0:c1] = sc.cpu().numpy()
        if world > 1:   # disjoint ranges, zeros elsewhere: the sum puts every range in place exactly
            out = parallel.allreduce_sum_(torch.from_numpy(out).cuda()).cpu().numpy()
        return out

    # ---- calibration (EmbeddingModel.py:2212-2575) ----
    def calibrate(self, X_pos, X_neg=None, positive_base_rate=None, batches_count=100, epochs=50):
        """Platt scaling of the model's scores on frozen embeddings (EmbeddingModel.py:2289-2535, AmpliGraph 1.x's ``calibrate``):
        fits ``calibration_parameters = [w, b]`` of ``predict_proba``'s sigmoid(-(w * score + b)) on the RAW score (no
        ``non_linearity`` link, no FocusE weight: :2245-2258).

        With ``X_neg`` (:2262-2287) the weighted cross-entropy over both sets is minimised to its minimiser (Newton on the
        device's moments; AmpliGraph: L-BFGS), the base rate defaulting to the sets' proportion (:2421-2424).  Without it
        (:2212-2260) every batch of ``X_pos`` — the ``batches_count`` contiguous slices ``fit`` would take — is corrupted afresh
        (eta = 1, 's,o', all entities) at each of the ``epochs`` x ``batches_count`` Adam steps (Keras defaults, :2509), and
        ``positive_base_rate`` is required (:2426-2432).  Labels, weights and start: :2439-2499; the sample weights are
        tf.losses.sigmoid_cross_entropy's (the reference's port dropped them)."""
        if not self.is_fitted:   # :2394-2397
            msg = "Model has not been fitted."
            logger.error(msg)
            raise RuntimeError(msg)
        if self.dealing_with_large_graphs:   # :2399-2402
            msg = "Calibration is incompatible with large graph mode."
            logger.error(msg)
            raise ValueError(msg)
        if positive_base_rate is not None and (positive_base_rate <= 0 or positive_base_rate >= 1):   # :2404-2409
            msg = "positive_base_rate must be a value between 0 and 1."
            logger.error(msg)
            raise ValueError(msg)
        if X_neg is None:
            self._refuse_without_kernel("calibrate without X_neg")
        if X_neg is None and positive_base_rate is None:   # :2426-2432
            msg = ("When calibrating with randomly generated negative corruptions, "
                   "`positive_base_rate` must be set to a value between 0 and 1.")
            logger.error(msg)
            raise ValueError(msg)
        x_pos = np.ascontiguousarray(to_idx(X_pos, ent_to_idx=self.ent_to_idx, rel_to_idx=self.rel_to_idx), dtype=np.int32)
        x_neg = None
        if X_neg is not None:
            x_neg = np.ascontiguousarray(to_idx(X_neg, ent_to_idx=self.ent_to_idx, rel_to_idx=self.rel_to_idx), dtype=np.int32)
            if len(x_pos) == 0 or len(x_neg) == 0:
                raise ValueError("calibrate needs at least one positive and one negative triple")
            if positive_base_rate is None:   # :2422-2423
                positive_base_rate = len(x_pos) / (len(x_pos) + len(x_neg))
        else:
            batches_count, epochs = int(batches_count), int(epochs)
            if batches_count < 1 or epochs < 0:
                raise ValueError("batches_count must be positive and epochs non-negative")
            if batches_count > len(x_pos):   # (the reference would average a loss over an empty batch)
                msg = "batches_count ({}) is larger than the number of positive triples ({}).".format(batches_count, len(x_pos))
                logger.error(msg)
                raise ValueError(msg)
        from .. import calibration as K
        ent, rel = self._device_tables()
        if x_neg is not None:
            w, b = K.calibrate_with_negatives(self._model_id(), ent, rel, self.internal_k, self._scale(), x_pos, x_neg,
                                              float(positive_base_rate))
        else:
            w, b = K.calibrate_with_corruptions(self._model_id(), ent, rel, self.internal_k, self._scale(), x_pos,
                                                float(positive_base_rate), batches_count, epochs, self.seed,
                                                verbose=self.verbose)
        self.calibration_parameters = [np.float32(w), np.float32(b)]   # :2531-2532
        self.is_calibrated = True

    def predict_proba(self, X, from_idx=False):
        """Probability of each triple of X to be true under the Platt scaling ``calibrate`` fitted (EmbeddingModel.py:2537-2575):
        sigmoid(-(w * score + b)) of the raw score, float32 [n]."""
        if not self.is_calibrated:   # :2548-2551
            msg = "Model has not been calibrated. Please call `model.calibrate(...)` before predicting probabilities."
            logger.error(msg)
            raise RuntimeError(msg)
        if type(X) is not np.ndarray:
            X = np.array(X)
        if X.ndim == 1:
            X = X[np.newaxis, :]
        if not from_idx:
            X = to_idx(X, ent_to_idx=self.ent_to_idx, rel_to_idx=self.rel_to_idx)
        X = np.ascontiguousarray(X, dtype=np.int32)
        from .. import calibration as K
        ent, rel = self._device_tables()
        w, b = self.calibration_parameters
        return K.predict_proba(self._model_id(), ent, rel, self.internal_k, self._scale(), X, w, b)

    _calibrate = calibrate            # the reference's names (:2289, :2537)
    _predict_proba = predict_proba

    # ---- evaluation protocol plumbing (EmbeddingModel.py:1494-1518,2035-2099) ----
    def set_filter_for_eval(self):
        """Configures to use filter (:1494-1496)."""
        self.is_filtered = True

    def configure_evaluation_protocol(self, config=None):
        """:1498-1518: keys corruption_entities ('all' | ids), corrupt_side, ranking_strategy."""
        if config is None:
            config = {"corruption_entities": DEFAULT_CORRUPTION_ENTITIES, "corrupt_side": DEFAULT_CORRUPT_SIDE_EVAL}
        self.eval_config = config

    def end_evaluation(self):
        """:2035-2044."""
        handle = getattr(self, "eval_dataset_handle", None)
        if self.is_filtered and handle is not None:
            handle.cleanup()
        self.eval_dataset_handle = None
        self.is_filtered = False
        self.eval_config = {}

    _ranks_as_array = True   # (evaluate_performance: get_ranks(..., as_array=True) is understood)

    def get_ranks(self, dataset_handle, as_array=False):
        """Ranks of the adapter's 'test' triples under the configured protocol (EmbeddingModel.py:2046-2099, with the
        intended one-rank-per-test-triple semantics, SURVEY A-1).  The filter comes from the adapter: its FilterIndex
        when it is this package's NumpyDatasetAdapter, otherwise the per-triple lists its
        get_next_batch(-1, 'test', use_filter=True) yields (the protocol of numpy_adapter.py:79-131).
        Returns the reference's Python lists; ``as_array=True`` (this package's evaluate_performance, which turns the lists
        into an array at once: building 4096 two-element lists and parsing them back was 1.6 of a 10.8 ms call) the int64 array."""
        if not self.is_fitted:
            msg = "Model has not been fitted."
            logger.error(msg)
            raise RuntimeError(msg)
        self.eval_dataset_handle = dataset_handle
        cfg = self.eval_config
        corrupt_side = cfg.get("corrupt_side", DEFAULT_CORRUPT_SIDE_EVAL)
        strategy = cfg.get("ranking_strategy", DEFAULT_RANK_COMPARE_STRATEGY)
        subset = cfg.get("corruption_entities", DEFAULT_CORRUPTION_ENTITIES)
        subset = None if isinstance(subset, str) else np.asarray(subset)
        findex = None
        if self.is_filtered:
            findex = getattr(dataset_handle, "filter_index", None)
        if self.is_filtered and findex is None:
            # a foreign adapter: collect its per-triple filter lists into the filter triples they stand for
            X_parts, rows = [], []
            for out in dataset_handle.get_next_batch(-1, "test", use_filter=True):
                x, objs, subs = np.asarray(out[0]).reshape(-1, 3), np.asarray(out[-2]).reshape(-1), np.asarray(out[-1]).reshape(-1)
                X_parts.append(x)
                rows.append(np.stack([np.full(len(objs), x[0, 0]), np.full(len(objs), x[0, 1]), objs], 1))
                rows.append(np.stack([subs, np.full(len(subs), x[0, 1]), np.full(len(subs), x[0, 2])], 1))
            X_idx = np.concatenate(X_parts, 0) if X_parts else np.zeros((0, 3), np.int64)
            findex = FilterIndex(np.concatenate(rows, 0)) if rows else None
        else:
            parts = [np.asarray(b[0] if isinstance(b, (list, tuple)) else b).reshape(-1, 3)
                     for b in dataset_handle.get_next_batch(1, "test")]
            X_idx = np.concatenate(parts, 0) if parts else np.zeros((0, 3), np.int64)
        ranks = self.get_ranks_idx(X_idx, filter_idx=findex, corrupt_side=corrupt_side, ranking_strategy=strategy,
                                   corruption_entities=subset, type_constraints=cfg.get("type_constraints"),
                                   candidates=cfg.get("candidates"), candidates_seed=cfg.get("candidates_seed", 0))
        if as_array:
            return ranks
        return [list(r) for r in ranks] if corrupt_side == "s,o" else list(ranks)

    def get_ranks_idx(self, X_idx, filter_idx=None, corrupt_side=DEFAULT_CORRUPT_SIDE_EVAL,
                      ranking_strategy=DEFAULT_RANK_COMPARE_STRATEGY, corruption_entities=None, verbose=False,
                      type_constraints=None, candidates=None, candidates_seed=0):
        """get_ranks (EmbeddingModel.py:2046-2099) on integer ids, intended per-triple semantics.  ``type_constraints`` (a
        TypeConstraints): typed ranks — every side among the pool of its relation (rank_triples_device says what that means
        and what it refuses); ``eval_precision`` 'auto', 0 and 2 give the same exact ranks, an explicit 1 is refused.
        ``candidates`` (an int K, or {'s' / 'o': int ids [n, K]}) with ``candidates_seed``: sampled ranks — every triple against
        a candidate list of its own (rank_triples_device: the semantics and the refusals)."""
        if not self.is_fitted:
            msg = "Model has not been fitted."
            logger.error(msg)
            raise RuntimeError(msg)
        self._refuse_ranking_under_link("ranking (get_ranks, evaluate_performance)")
        self._refuse_without_kernel("ranking")
        link = self._rank_link_id()
        from ..evaluation.ranking import derived_tables, resolve_rank_mode
        shard = parallel.rank_world() if parallel.is_active() else None
        if self.embedding_model_params.get("sharding"):
            if candidates is not None:
                raise NotImplementedError("ranking against candidate lists runs on one GPU: embedding_model_params['sharding'] is not "
                                          "available with it")
            if type_constraints is not None:
                raise NotImplementedError("typed ranking runs on one GPU: embedding_model_params['sharding'] is not available with it")
        # lists and typed ranking: every refusal before the device is asked for (their rules do not read the table's size)
        n_ent = 0 if candidates is not None or type_constraints is not None else int(self._device_tables()[0].shape[0])
        mode = resolve_rank_mode(self._model_id(), self.internal_k, int(np.asarray(X_idx).reshape(-1, 3).shape[0]), n_ent,
                                 self._eval_precision(), link, shard, corruption_entities, type_constraints, candidates, corrupt_side,
                                 ranking_strategy)   # (the call below decides the same mode from the same arguments)
        ent, rel = self._device_tables()
        tables = None
        if mode.path == "exact_fast":
            # what the exact-fast mode derives from the tables (half-precision copy, norm bounds, ...) is kept with the
            # device copy of the fitted parameters: repeated evaluations of a fitted model do not rebuild it (0.63 M -> 0.75 M
            # ranks/s at |E| = 1M, bench `eval.exact_fast.*.uncached_tables`); a new fit / restore replaces both
            # (after fit() the device tables may be the trainer's LIVE ones: keyed on its step count too, so that further steps —
            # early stopping's evaluations between epochs, a caller driving the trainer — never meet stale half-precision copies)
            tr = getattr(self, "_trainer", None)
            stamp = (self._dev, tr.step_count if tr is not None else -1)
            cached = getattr(self, "_derived_cache", None)
            if cached is None or cached[0][0] is not stamp[0] or cached[0][1] != stamp[1]:
                cached = self._derived_cache = (stamp, derived_tables(self._model_id(), ent, rel, self.internal_k))
            tables = cached[1]
        return rank_triples_device(self._model_id(), ent, rel, self.internal_k, self._scale(), X_idx, corrupt_side,
                                   ranking_strategy, filter_triples=filter_idx, entities_subset=corruption_entities, shard=shard,
                                   precision=self._eval_precision(), ent_f16=tables, link=link, type_constraints=type_constraints,
                                   candidates=mode.candidates, candidates_seed=candidates_seed)

    def get_topn_idx(self, X_idx, side="o", top_n=10, filter_idx=None, corruption_entities=None):
        """The top_n best completions of the queries X_idx (int ids [n, 2]: (s, p) for side 'o', (p, o) for side 's'), among
        all entities or ``corruption_entities``, the known completions of ``filter_idx`` (int triples or a FilterIndex)
        excluded: (ids int32 [n, top_n], scores float32 [n, top_n]), short rows padded with (-1, -inf).  The order is the
        raw score's (ties by ascending id); the returned scores carry the link of predict (EmbeddingModel.py:2135-2145)."""
        from ..evaluation.ranking import check_top_n, topn_device
        top_n = check_top_n(top_n)
        if side not in ("s", "o"):
            raise ValueError("side must be 's' or 'o'")
        if not self.is_fitted:
            msg = "Model has not been fitted."
            logger.error(msg)
            raise RuntimeError(msg)
        link = self._link()
        X_idx = np.asarray(X_idx)
        if X_idx.ndim != 2 or X_idx.shape[1] != 2:
            raise ValueError("X must have shape [n, 2]")
        ent, rel = self._device_tables()
        ids, scores = topn_device(self._model_id(), ent, rel, self.internal_k, self._scale(), X_idx, side, top_n,
                                  filter_triples=filter_idx, entities_subset=corruption_entities)
        if link != "linear":   # non-decreasing: the raw order stands (padding: -inf stays the lowest value of each link)
            pad = ids < 0
            sc = torch.from_numpy(scores)
            if link == "tanh":
                sc = torch.tanh(sc)
            elif link == "sigmoid":
                sc = torch.sigmoid(sc)
            elif link == "softplus":
                sc = torch.log(1 + 9999 * torch.exp(sc))   # custom_softplus, :90-96
            scores = sc.numpy()
            scores[pad] = -np.inf
        return ids, scores

    def _refuse_relation_side_sharded(self, what):
        """the relation-side kernels run on one GPU"""
        if self.embedding_model_params.get("sharding") or parallel.is_active():
            raise NotImplementedError("{} runs on one GPU: sharded or multi-GPU use is not available".format(what))

    def get_relation_ranks_idx(self, X_idx, filter_idx=None, ranking_strategy=DEFAULT_RANK_COMPARE_STRATEGY,
                               corruption_relations=None):
        """Relation-side ranks of the triples X_idx (int ids [n, 3]): the rank of p among all relations (or
        ``corruption_relations``) completing (s, ?, o), int64 [n]; ``filter_idx`` (int triples or a FilterIndex): the known
        relations of the pair other than p do not count.  Not in the reference; a triple's score is the one the
        object side ranks (rank_relations_device).  One exact kernel: ``eval_precision`` is not consulted.  A non-linear
        ``non_linearity`` is refused or ranked through exactly as get_ranks_idx does (``rank_through_link``)."""
        if not self.is_fitted:
            msg = "Model has not been fitted."
            logger.error(msg)
            raise RuntimeError(msg)
        self._refuse_ranking_under_link("relation ranking (get_relation_ranks_idx, evaluate_relation_prediction)")
        self._refuse_relation_side_sharded("relation ranking")
        X_idx = np.asarray(X_idx)
        if X_idx.ndim != 2 or X_idx.shape[1] != 3:
            raise ValueError("X must have shape [n, 3]")
        from ..evaluation.ranking import rank_relations_device
        ent, rel = self._device_tables()
        return rank_relations_device(self._model_id(), ent, rel, self.internal_k, self._scale(), X_idx, ranking_strategy,
                                     filter_triples=filter_idx, relations_subset=corruption_relations, link=self._rank_link_id())

    def get_topn_relations_idx(self, X_idx, top_n=10, filter_idx=None, corruption_relations=None):
        """The top_n best relations between the pairs X_idx (int ids [n, 2] = (s, o)), among all relations or
        ``corruption_relations``, the known relations of ``filter_idx`` (int triples or a FilterIndex) excluded:
        (ids int32 [n, top_n], scores float32 [n, top_n]), short rows padded with (-1, -inf).  The order is the raw score's (ties
        by ascending id); the returned scores carry the link of predict (EmbeddingModel.py:2135-2145), as get_topn_idx's."""
        from ..evaluation.ranking import check_top_n, topn_relations_device
        top_n = check_top_n(top_n)
        if not self.is_fitted:
            msg = "Model has not been fitted."
            logger.error(msg)
            raise RuntimeError(msg)
        self._refuse_relation_side_sharded("topn_relations")
        link = self._link()
        X_idx = np.asarray(X_idx)
        if X_idx.ndim != 2 or X_idx.shape[1] != 2:
            raise ValueError("X must have shape [n, 2]")
        ent, rel = self._device_tables()
        ids, scores = topn_relations_device(self._model_id(), ent, rel, self.internal_k, self._scale(), X_idx, top_n,
                                            filter_triples=filter_idx, relations_subset=corruption_relations)
        if link != "linear":   # non-decreasing: the raw order stands (padding: -inf stays the lowest value of each link)
            pad = ids < 0
            sc = torch.from_numpy(scores)
            if link == "tanh":
                sc = torch.tanh(sc)
            elif link == "sigmoid":
                sc = torch.sigmoid(sc)
            elif link == "softplus":
                sc = torch.log(1 + 9999 * torch.exp(sc))   # custom_softplus, :90-96
            scores = sc.numpy()
            scores[pad] = -np.inf
        return ids, scores

    def _eval_precision(self):
        """embedding_model_params['eval_precision'] / EMG_EVAL_PRECISION: 0 exact f32 kernel, 2 exact ranks through the
        half-precision MFMA prefilter (bit-equal to 0), 1 bf16 throughput mode (statistical agreement only: never picked
        implicitly), 'auto' (default) = 2 where it applies and pays, else 0."""
        v = self.embedding_model_params.get("eval_precision", _switches.get("EMG_EVAL_PRECISION"))
        if v in ("auto", 0, 1, 2):
            return v
        if str(v) in ("0", "1", "2"):
            return int(v)
        raise ValueError("eval_precision must be 0, 1, 2 or 'auto', got {!r}".format(v))


@register_model("TransE")
class TransE(EmbeddingModel):
    """TransE (TransE.py): f = -||e_s + r_p - e_o||_n, n = embedding_model_params['norm'] in {1, 2}."""

    def __init__(self, k=DEFAULT_EMBEDDING_SIZE, eta=DEFAULT_ETA, epochs=DEFAULT_EPOCH,
                 batches_count=DEFAULT_BATCH_COUNT, seed=DEFAULT_SEED,
                 embedding_model_params={"norm": DEFAULT_NORM_TRANSE, "normalize_ent_emb": DEFAULT_NORMALIZE_EMBEDDINGS,
                                         "negative_corruption_entities": DEFAULT_CORRUPTION_ENTITIES,
                                         "corrupt_sides": DEFAULT_CORRUPT_SIDE_TRAIN},
                 optimizer=DEFAULT_OPTIM, optimizer_params={"lr": DEFAULT_LR}, loss=DEFAULT_LOSS, loss_params={},
                 regularizer=DEFAULT_REGULARIZER, regularizer_params={}, initializer=DEFAULT_INITIALIZER,
                 initializer_params={"uniform": DEFAULT_GLOROT_IS_UNIFORM}, verbose=DEFAULT_VERBOSE,
                 large_graphs=False):
        super().__init__(k=k, eta=eta, epochs=epochs, batches_count=batches_count, seed=seed,
                         embedding_model_params=embedding_model_params, optimizer=optimizer,
                         optimizer_params=optimizer_params, loss=loss, loss_params=loss_params,
                         regularizer=regularizer, regularizer_params=regularizer_params, initializer=initializer,
                         initializer_params=initializer_params, verbose=verbose, large_graphs=large_graphs)

    def _norm(self):
        norm = self.embedding_model_params.get("norm", DEFAULT_NORM_TRANSE)
        if norm == "euclidean":
            norm = 2
        try:
            ok = float(norm) > 0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("TransE norm {!r}: expected a positive order of the vector norm (1, 2, ..., np.inf)".format(norm))
        return norm

    def _model_id(self):
        """norm 1 / 2: the tuned models; any other positive order (TransE.py:208-216 passes `norm` to tf.norm as ord): EMG_TRANSE_P —
        generic kernels for fit (unfused forward / loss / backward), predict, get_ranks and evaluate_performance (exact path)"""
        norm = self._norm()
        return L.TRANSE_L1 if norm == 1 else (L.TRANSE_L2 if norm == 2 else L.TRANSE_P)

    def _scale(self):
        return float(self._norm()) if self._model_id() == L.TRANSE_P else 1.0



@register_model("DistMult")
class DistMult(EmbeddingModel):
    """DistMult (DistMult.py): f = <r_p, e_s, e_o>."""

    def __init__(self, k=DEFAULT_EMBEDDING_SIZE, eta=DEFAULT_ETA, epochs=DEFAULT_EPOCH,
                 batches_count=DEFAULT_BATCH_COUNT, seed=DEFAULT_SEED,
                 embedding_model_params={"normalize_ent_emb": DEFAULT_NORMALIZE_EMBEDDINGS,
                                         "negative_corruption_entities": DEFAULT_CORRUPTION_ENTITIES,
                                         "corrupt_sides": DEFAULT_CORRUPT_SIDE_TRAIN},
                 optimizer=DEFAULT_OPTIM, optimizer_params={"lr": DEFAULT_LR}, loss=DEFAULT_LOSS, loss_params={},
                 regularizer=DEFAULT_REGULARIZER, regularizer_params={}, initializer=DEFAULT_INITIALIZER,
                 initializer_params={"uniform": DEFAULT_GLOROT_IS_UNIFORM}, verbose=DEFAULT_VERBOSE):
        super().__init__(k=k, eta=eta, epochs=epochs, batches_count=batches_count, seed=seed,
                         embedding_model_params=embedding_model_params, optimizer=optimizer,
                         optimizer_params=optimizer_params, loss=loss, loss_params=loss_params,
                         regularizer=regularizer, regularizer_params=regularizer_params, initializer=initializer,
                         initializer_params=initializer_params, verbose=verbose)

    def _model_id(self):
        return L.DISTMULT



@register_model("ComplEx")
class ComplEx(EmbeddingModel):
    """ComplEx (ComplEx.py): f = Re(<r_p, e_s, conj(e_o)>); rows are [re | im], internal_k = 2k (:224)."""
    _pair_rows = True

    def __init__(self, k=DEFAULT_EMBEDDING_SIZE, eta=DEFAULT_ETA, epochs=DEFAULT_EPOCH,
                 batches_count=DEFAULT_BATCH_COUNT, seed=DEFAULT_SEED,
                 embedding_model_params={"negative_corruption_entities": DEFAULT_CORRUPTION_ENTITIES,
                                         "corrupt_sides": DEFAULT_CORRUPT_SIDE_TRAIN},
                 optimizer=DEFAULT_OPTIM, optimizer_params={"lr": DEFAULT_LR}, loss=DEFAULT_LOSS, loss_params={},
                 regularizer=DEFAULT_REGULARIZER, regularizer_params={}, initializer=DEFAULT_INITIALIZER,
                 initializer_params={"uniform": DEFAULT_GLOROT_IS_UNIFORM}, verbose=DEFAULT_VERBOSE):
        super().__init__(k=k, eta=eta, epochs=epochs, batches_count=batches_count, seed=seed,
                         embedding_model_params=embedding_model_params, optimizer=optimizer,
                         optimizer_params=optimizer_params, loss=loss, loss_params=loss_params,
                         regularizer=regularizer, regularizer_params=regularizer_params, initializer=initializer,
                         initializer_params=initializer_params, verbose=verbose)
        self.internal_k = self.k * 2

    def _model_id(self):
        return L.COMPLEX



@register_model("HolE")
class HolE(ComplEx):
    """HolE (HolE.py:189): f = (2/k) * f_ComplEx (Hayashi & Shimbo equivalence; NOT an FFT, SURVEY A-12)."""

    def _model_id(self):
        return L.HOLE

    def _scale(self):
        return float(np.float32(2 / self.k))



@register_model("RotatE")
class RotatE(ComplEx):
    """RotatE (Sun et al., ICLR 2019; not in the reference: DESIGN.md 0, A-22): f = -sum_j |e_s,j r_j - e_o,j|, r_j = exp(i theta_j) — the
    paper's L1-of-moduli score without the constant gamma, which is the losses' ``margin``.  Entity rows are [re | im], internal_k =
    2k; a relation row has the same width, columns [0, k) the phases theta (uniform in [-pi, pi) from the model's seed), columns
    [k, 2k) unused and zero.  ``get_embeddings(..., 'relation')`` returns the k phases.  Constructor: ComplEx's.

    Runs on one GPU through the generic kernels (include/emgraph_hip.h, EMG_ROTATE): fit with every loss, optimizer and regulariser,
    early stopping, predict, get_ranks / evaluate_performance (eval_precision 0: the exact kernel; 'auto', the default: the exact-fast
    mode — half-precision prefilter, exact re-scoring, the same ranks bit for bit — for at least 128 triples against at least 32768
    entities without a candidate list, else the exact kernel; under rank_through_link always the exact kernel), rank_through_link,
    topn_completions, save / restore, calibrate(X_pos, X_neg) / predict_proba, the entity-mode discovery calls.  NotImplementedError:
    sharding of any kind, eval_precision 1 / 2 (the exact-fast mode is reached through 'auto'; a later change that may edit the tests
    pinning this refusal can open an explicit 2), discover_facts and calibrate without X_neg (kernels with scoring loops of their own)."""

    _phase_relations = True

    def _model_id(self):
        return L.ROTATE

    def _initial_relation_table(self, n_rel, dev, rnd=None):
        """phases uniform in [-pi, pi) in columns [0, k) (the device init routine, the model's seed, whatever the entity initializer);
        columns [k, 2k) zero.  The 'constant' initializer's relation array is taken as it is: phases in its first k columns."""
        if rnd is not None:
            return super()._initial_relation_table(n_rel, dev, rnd)
        t = alloc_table(n_rel, self.internal_k, dev)
        D.init_table(t, self.k, "uniform", -np.pi, np.pi, self.seed, 2)
        return t

    def _refuse_without_kernel(self, what):
        p = self.embedding_model_params
        sharding = p.get("sharding")   # (asked for at all: the same answer on any box, as for FocusE)
        asked = ("embedding_model_params['sharding'] = {!r}".format(sharding) if sharding else
                 ("predict(sharded=True)" if what == "predict(sharded=True)" else ("a multi-GPU job" if parallel.is_active() else None)))
        if asked:
            raise NotImplementedError("RotatE runs on one GPU: sharding ({}) is not available".format(asked))
        if what in ("fit", "ranking") and self._eval_precision() in (1, 2):
            raise NotImplementedError("RotatE is ranked by the exact kernel: eval_precision must be 0 or 'auto', got {!r}".format(
                self._eval_precision()))
        if what in ("discover_facts", "calibrate without X_neg"):
            raise NotImplementedError("RotatE: {} is not available (its kernel has a scoring loop of its own, without a RotatE "
                                      "form){}".format(what, "; pass X_neg" if what.startswith("calibrate") else ""))

    def get_embeddings(self, entities, embedding_type="entity"):
        emb = super().get_embeddings(entities, embedding_type)
        return emb[..., :self.k] if embedding_type == "relation" else emb


@register_model("SimplE")
class SimplE(ComplEx):
    """SimplE (Kazemi & Poole, NeurIPS 2018; not in the reference: DESIGN.md 0, A-27, 4.6), the averaged form: an entity row is [h | t]
    (the entity as a head and as a tail), a relation row [r | r_inv], internal_k = 2k, and
    f(s, p, o) = 1/2 (<h_s, r, t_o> + <h_o, r_inv, t_s>).  Fully expressive; models asymmetric relations, which DistMult cannot.
    Both tables come from the model's initializer; ``get_embeddings`` returns the whole 2k row.  Constructor: ComplEx's.

    A 1-vs-all score is a 2k-wide dot product of a query row with an entity row, times 1/2 — the scaled contraction chain of HolE on
    SimplE's own query rows — so ranking takes every path ComplEx takes at ComplEx's speed: eval_precision 0, 1, 2 and 'auto' (the
    exact-fast default), rank_through_link, type_constraints, candidates, corruption_entities, topn_completions,
    evaluate_relation_prediction / topn_relations, discover_facts and the entity-mode discovery calls, calibrate(X_pos, X_neg) /
    predict_proba, save / restore.  Training runs on one GPU through the generic kernels (include/emgraph_hip.h, EMG_SIMPLE): every
    loss, optimizer and regulariser, score links, FocusE, early stopping, every negative-sampling option but shared negatives.
    NotImplementedError: sharding of any kind, embedding_model_params['shared_negatives'], calibrate without X_neg."""

    _pair_rows = False   # ([h | t] rows: not complex coordinates)

    def _model_id(self):
        return L.SIMPLE

    def _scale(self):
        return 0.5

    def _refuse_without_kernel(self, what):
        p = self.embedding_model_params
        sharding = p.get("sharding")   # (asked for at all: the same answer on any box, as for FocusE)
        asked = ("embedding_model_params['sharding'] = {!r}".format(sharding) if sharding else
                 ("predict(sharded=True)" if what == "predict(sharded=True)" else ("a multi-GPU job" if parallel.is_active() else None)))
        if asked:
            raise NotImplementedError("SimplE runs on one GPU: sharding ({}) is not available".format(asked))
        if what == "fit" and "shared_negatives" in p:
            raise NotImplementedError("SimplE: embedding_model_params['shared_negatives'] is not available (the shared-negatives "
                                      "kernels have no SimplE form)")
        if what == "calibrate without X_neg":
            raise NotImplementedError("SimplE: calibrate without X_neg is not available (its kernel has a scoring loop of its own, "
                                      "without a SimplE form); pass X_neg")
