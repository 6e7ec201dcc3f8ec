"""tda-multimodal_amd: MI355X-native drop-in for the reference's ripser hot path.

Import with ``importlib.import_module("tda-multimodal_amd")`` (the directory
name carries a hyphen); the package registers itself as ``tda_multimodal_amd``
too.  Product path = libtda_rips.so (HIP, gfx950) via the C ABI in
include/tda_rips.h; no CPU fallback.
"""
import sys as _sys

from . import bootstrap, diagrams, distributed, geodesic, hypothesis, metrics, phdim, synthetic, umap  # noqa: F401
from .bootstrap import ConfidenceBands, confidence_bands, hausdorff_resamples, resample_indices  # noqa: F401
from .diagrams import (betti_curve, betti_curves, bottleneck, bottleneck_matrix, entropy_curve, entropy_curves, fisher,  # noqa: F401
                       fisher_kernel_matrix, fisher_matrix, heat, heat_kernel_matrix, heat_matrix, lifespan_curve, lifespan_curves, persistence_curves, persistence_image, persistence_images,
                       persistence_landscape, persistence_landscapes, persistence_silhouette, persistence_silhouettes, sliced_wasserstein,
                       sliced_wasserstein_kernel, sliced_wasserstein_matrix, wasserstein, wasserstein_matrix)
from .geodesic import GeodesicDistances, geodesic_distances  # noqa: F401
from .phdim import PHDimension, h0_subsamples, ph_dimension, subsample_indices  # noqa: F401
from .hypothesis import PermutationTest, diagram_permutation_test, label_permutations, permutation_test  # noqa: F401
from .metrics import (compute_effective_dimensionality, compute_fixed_window_ed, compute_fixed_window_id,  # noqa: F401
                      compute_intrinsic_dimensionality, matrix_entropy, matrix_entropy_profile)
from ._lib import BOTTLENECK_EXPORTS, CURVE_EXPORTS, DGM_EXPORTS, EXPORTS, FISHER_EXPORTS, HEAT_EXPORTS, LIB_PATH, SUBSAMPLE_H0_EXPORTS, VECTOR_EXPORTS, WASSERSTEIN_EXPORTS, build, lib  # noqa: F401
from .pipeline import (get_max_persistence, get_persistence, layer_distance_matrix, layer_features, layer_record,  # noqa: F401
                       layer_record_adversarial, peak_layer, run_adversarial_condition, run_sweep, write_layer_stats,
                       write_summary_stats)
from .umap import UMAP, umap_batch, umap_transform_batch  # noqa: F401
from .ripser import (GreedyPerm, LayerResult, SweepPipeline, greedy_perm, greedy_perm_batch, persistence_pairs, ripser,  # noqa: F401
                     ripser_batch, rips_dm, silhouette_score)

_sys.modules.setdefault("tda_multimodal_amd", _sys.modules[__name__])

__all__ = [
    "ripser",
    "ripser_batch",
    "SweepPipeline",
    "rips_dm",
    "persistence_pairs",
    "LayerResult",
    "greedy_perm",
    "greedy_perm_batch",
    "GreedyPerm",
    "get_persistence",
    "get_max_persistence",
    "layer_record",
    "layer_record_adversarial",
    "run_adversarial_condition",
    "run_sweep",
    "write_summary_stats",
    "peak_layer",
    "layer_distance_matrix",
    "sliced_wasserstein",
    "sliced_wasserstein_matrix",
    "sliced_wasserstein_kernel",
    "bottleneck",
    "bottleneck_matrix",
    "wasserstein",
    "wasserstein_matrix",
    "heat",
    "heat_matrix",
    "heat_kernel_matrix",
    "fisher",
    "fisher_matrix",
    "fisher_kernel_matrix",
    "layer_features",
    "confidence_bands",
    "ConfidenceBands",
    "resample_indices",
    "hausdorff_resamples",
    "ph_dimension",
    "PHDimension",
    "h0_subsamples",
    "subsample_indices",
    "geodesic_distances",
    "GeodesicDistances",
    "permutation_test",
    "diagram_permutation_test",
    "label_permutations",
    "PermutationTest",
    "persistence_landscape",
    "persistence_landscapes",
    "persistence_image",
    "persistence_images",
    "persistence_curves",
    "betti_curve",
    "betti_curves",
    "lifespan_curve",
    "lifespan_curves",
    "entropy_curve",
    "entropy_curves",
    "persistence_silhouette",
    "persistence_silhouettes",
    "silhouette_score",
    "compute_intrinsic_dimensionality",
    "compute_effective_dimensionality",
    "compute_fixed_window_ed",
    "compute_fixed_window_id",
    "matrix_entropy",
    "matrix_entropy_profile",
    "UMAP",
    "umap_batch",
    "umap_transform_batch",
    "build",
    "lib",
]
