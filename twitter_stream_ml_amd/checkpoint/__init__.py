"""Model checkpoints in MLlib's Saveable layout (metadata JSON + parquet) + stream positions."""
from .saveable import (KMEANS_CLASS, LOGISTIC_CLASS, LR_CLASS, SparseWeights, load_kmeans, load_linear_regression,
                       load_logistic_regression, load_progress, model_class, save_kmeans, save_linear_regression,
                       save_logistic_regression, vector_udt_type)
from .stream_state import StreamPositions, resolve_resume

__all__ = ["KMEANS_CLASS", "LOGISTIC_CLASS", "LR_CLASS", "SparseWeights", "load_kmeans", "load_linear_regression",
           "load_logistic_regression", "load_progress", "model_class", "save_kmeans", "save_linear_regression",
           "save_logistic_regression", "vector_udt_type", "StreamPositions", "resolve_resume"]
