"""Mirrors emgraph/evaluation/__init__.py exports for the hot path."""
from .metrics import hits_at_n_score, mr_score, mrr_score, rank_score
from .protocol import (check_filter_size, create_mappings, evaluate_performance, filter_unseen_entities,
                       evaluate_relation_prediction, generate_corruptions_for_eval, generate_corruptions_for_fit, to_idx,
                       topn_completions, topn_relations)
from .ranking import (FilterIndex, L2Tables, PrefilterTables, SadTables, build_filter_csr, grid_ranks_device, rank_triples_device,
                      rank_relations_device, ranks_from_counts, topn_device, topn_relations_device)
from ..type_constraints import TypeConstraints

__all__ = ["hits_at_n_score", "mr_score", "mrr_score", "rank_score", "check_filter_size", "create_mappings",
           "evaluate_performance", "filter_unseen_entities", "generate_corruptions_for_eval",
           "generate_corruptions_for_fit", "to_idx", "topn_completions", "topn_device", "FilterIndex", "PrefilterTables", "SadTables", "L2Tables", "build_filter_csr", "rank_triples_device",
           "ranks_from_counts", "grid_ranks_device", "evaluate_relation_prediction", "topn_relations", "rank_relations_device",
           "topn_relations_device", "TypeConstraints"]
