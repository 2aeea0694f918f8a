"""modl_amd — MI355X-native implementation of MODL's SOMF hot path
(DictFact.partial_fit: code solve, surrogate statistics, block-coordinate
dictionary update) behind the reference's estimator API."""
from .dict_fact import DictFact, Coder, SparseCodes  # noqa: F401
from .stability import amari_discrepency, mean_amari_discrepency  # noqa: F401
from .image import grid_origins, grid_patches, reconstruct_from_patches  # noqa: F401
from .signal import clean, cleaning_basis, butterworth  # noqa: F401
from .masker import ArrayMasker, smooth_mask, unmask, gaussian_weights  # noqa: F401
from .masker import resample, resample_mask, resample_host, voxel_size_of  # noqa: F401
from .masker import (compute_epi_mask, compute_background_mask, compute_multi_epi_mask,  # noqa: F401
                     compute_multi_background_mask, intersect_masks, largest_connected_component)
from .regions import Regions, connected_regions, region_labels, connected_regions_host, region_labels_host  # noqa: F401
from .canica import (IcaMaps, Canica, reduce_record, group_components, fastica_maps, threshold_maps, canica,  # noqa: F401
                     reduce_record_host, group_components_host, fastica_maps_host, threshold_maps_host, canica_host)
from .connectivity import (covariances, ConnectivityMeasure, geometric_mean, sym_matrix_to_vec, vec_to_sym_matrix,  # noqa: F401
                           seed_correlation, covariances_host, ConnectivityMeasureHost, geometric_mean_host,
                           seed_correlation_host)
from .parcellation import (KMeansParcels, Parcellation, kmeans_init, kmeans_parcels, label_signals, signals_to_rows,  # noqa: F401
                           parcellate, kmeans_init_host, kmeans_parcels_host, label_signals_host, signals_to_rows_host,
                           parcellate_host)

__all__ = ['DictFact', 'Coder', 'SparseCodes', 'amari_discrepency', 'mean_amari_discrepency', 'grid_origins', 'grid_patches',
           'reconstruct_from_patches', 'clean', 'cleaning_basis', 'butterworth', 'ArrayMasker', 'smooth_mask', 'unmask',
           'gaussian_weights', 'resample', 'resample_mask', 'resample_host', 'voxel_size_of', 'compute_epi_mask',
           'compute_background_mask', 'compute_multi_epi_mask', 'compute_multi_background_mask', 'intersect_masks',
           'largest_connected_component', 'Regions', 'connected_regions', 'region_labels', 'connected_regions_host',
           'region_labels_host', 'IcaMaps', 'Canica', 'reduce_record', 'group_components', 'fastica_maps', 'threshold_maps',
           'canica', 'reduce_record_host', 'group_components_host', 'fastica_maps_host', 'threshold_maps_host', 'canica_host',
           'covariances', 'ConnectivityMeasure', 'geometric_mean', 'sym_matrix_to_vec', 'vec_to_sym_matrix', 'seed_correlation',
           'covariances_host', 'ConnectivityMeasureHost', 'geometric_mean_host', 'seed_correlation_host']
