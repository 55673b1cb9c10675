"""Mirrors emgraph/models/__init__.py for the hot-path models; RotatE and SimplE are this package's own."""
from .embedding_model import (MODEL_REGISTRY, ComplEx, DistMult, EmbeddingModel, HolE, RotatE, SimplE, TransE,
                              reset_entity_threshold, set_entity_threshold)

__all__ = ["EmbeddingModel", "TransE", "DistMult", "ComplEx", "HolE", "RotatE", "SimplE", "MODEL_REGISTRY", "set_entity_threshold",
           "reset_entity_threshold"]
