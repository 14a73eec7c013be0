from .knn import evaluate_knn, evaluate_knn_sharded, extract_features
from .linear import evaluate_linear_probe, evaluate_linear_sharded
from .segmentation import evaluate_segmentation_linear, extract_dense_features

__all__ = ["extract_features", "evaluate_knn", "evaluate_knn_sharded", "evaluate_linear_probe",
           "evaluate_linear_sharded", "evaluate_segmentation_linear", "extract_dense_features"]
