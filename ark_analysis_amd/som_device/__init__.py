"""Device-level SOM operations: thin, typed wrappers over the C ABI working on torch tensors.

Tensors are only device-memory holders here (``data_ptr()`` goes across the ABI); every
function launches on torch's current HIP stream and returns without synchronising.

The wrappers live in one module per kernel family; this file only names them, so that every caller goes on writing
``som_device.NAME``.  ``_args`` holds the argument checks and dtype tables the families share.
"""
from ._args import (PAIR_CAPACITY_MAX, PLANE_DTYPES, PLANE_MODE_DTYPES, SEG_DTYPES, SEG_F64, _binary_plane, _check_metric,
                    _codebook, _key_range, _label_image, _label_pair, _label_plane, _ld, _like_plane, _matrix_args,
                    _rows_plane)
from .som import (ACC_PREPARED, ASSIGN_SCREEN_ALL_LISTS, ONLINE_INT_ABS, ONLINE_LANES_PER_NODE, ONLINE_ROUTE_FIELDS,
                  ONLINE_THREAD_PER_NODE, TABLES_SCRATCH_CLEAN, TRAIN_UNFUSED, AssignSumsWorkspace, AssignWorkspace,
                  BatchTrainState, MetricStepWorkspace, absmax, assign, assign_means, assign_sums, assign_sums_metric,
                  batch_accumulate, batch_train_finish,
                  batch_train_fused_route, batch_train_steps, batch_update, batch_update_prepare, cluster_sums,
                  exact_sum_quantum, last_exact_rows, pair_histogram, relabel, train_online, train_online_route,
                  train_online_routes, _with_scratch_flag)
from .comm import COMM_ID_BYTES, P2P_HANDLE_BYTES, P2PComm, RankComm, _torch_rccl_path
from .pixels import (gaussian_blur_hwc, gaussian_kernel1d, normalize_columns, quantile_f32, quantile_nonzero,
                     rowsum_filter_normalize, scaled_rowsum, scaled_rowsum_f32, to_numpy)
from .planes import (BIN_LEVEL, BIN_LOCAL, BIN_POSITIVE, BLUR_MAX_RADIUS, BLUR_MODES, BLUR_SIGMA_LIMIT, CCL_TILE,
                     LUT_UNMAPPED, MASK_BAD_LABEL, MASK_BAD_PIXEL, RIDGE_MAX_RADIUS, RIDGE_MAX_SCALES,
                     SEGMASK_FORCE_SEARCH, SEG_ERODE, SELECT_FILL, SELECT_KEEP, binarize_plane, check_blur_sigma,
                     choose_merges, cluster_mask, components_select, gaussian_blur_plane, gaussian_blur_plane_mode,
                     label_components, label_regions, merge_apply, merge_masks, object_mask, pair_overlaps, ridge_sign,
                     segmask_table, segmentation_mask, zero_by_segmentation, _blur_plane, _region_tables)
from .planes import (EDT_NO_BACKGROUND, HISTOGRAM_MAX_BINS, class_markers, distance_transform_edt, histogram_edges,
                     plane_greater, plane_histogram, plane_minmax, sobel_magnitude, watershed_inputs)
from .planes import FRANGI_SIGMAS, GRADIENT_TOO_SMALL, frangi, frangi_arguments, ridge_watershed_inputs
from .planes import (CLAHE_GREY_LEVELS, CLAHE_NBINS, channel_watershed_inputs, clahe_arguments, contrast_adjust,
                     equalize_adapthist)
from .planes import WATERSHED_STATS, channel_fiber_labels, watershed
from .overlays import (COLORIZE_BAD_INDEX, COLORIZE_MASK_DTYPES, OVERLAY_CLIP, OVERLAY_RESCALE, OVERLAY_ZERO, colorize,
                       overlay_compose, overlay_ranges, overlay_rgb, percentiles_positive)
from .embedding import (TSNE_MAX_ROWS, TsneResult, column_moments, pair_sqdist_f32, pca_scores, principal_axes,
                        project_rows, tsne, tsne_affinities, tsne_embed, tsne_learning_rate, tsne_max_rows, tsne_step,
                        tsne_workspace_bytes)
from .cells import (CELLQUANT_FORCE_SEARCH, CELLQUANT_IMAGE_DTYPES, CELLQUANT_MODES, CELLQUANT_NUC_CAPACITY,
                    CONCAVITY_DEFAULTS, NUCSPLIT_FORCE_SEARCH, REGION_FORCE_SEARCH, REGION_MAX_SIDE, cell_quantify,
                    choose_splits, label_keys, nuclear_overlaps, region_euler, region_moments, region_props,
                    split_large_nuclei, split_nuclei_apply, _region_keys, _split_planes)
from .spatial import (CLOSE_PAIR_MAX_SETS, NEAREST_MAX_K, _S_ZERO, close_pair_counts, nearest_indices, nearest_type_means,
                      neighbor_counts, neighbor_thresholds, neighborhood_sums, radius_threshold, _cell_args, _cells_sorted_by_type, _check_offsets, _nearest_s_zero,
                      _smallest_double)
from .clustering import (KMEANS_MAX_D, KMEANS_MAX_K, KMEANS_MAX_PROBLEMS, SILHOUETTE_MAX_D, SILHOUETTE_MAX_K,
                         kmeans_group_count, kmeans_lloyd, silhouette_samples, silhouette_scores, silhouette_sums, _kmeans_ks, _silhouette,
                         _silhouette_call)
