"""som_device is a package of one module per kernel family behind a facade: every name the single module had at
326a4f9 (its top-level ``def``, ``class`` and assignment targets, by an AST pass over that file) stays reachable as
``som_device.NAME``, bound to the object the defining submodule holds.  No GPU and no libpxsom.so needed."""
import importlib
import inspect

PARENT_NAMES = (
    "_matrix_args", "_codebook", "AssignWorkspace", "_check_metric", "assign", "last_exact_rows", "cluster_sums",
    "TRAIN_UNFUSED", "ASSIGN_SCREEN_ALL_LISTS", "BatchTrainState", "absmax", "exact_sum_quantum",
    "batch_train_fused_route", "ONLINE_ROUTE_FIELDS", "ONLINE_LANES_PER_NODE", "ONLINE_THREAD_PER_NODE",
    "train_online_route", "train_online_routes", "batch_train_steps", "COMM_ID_BYTES", "_torch_rccl_path", "RankComm",
    "P2P_HANDLE_BYTES", "P2PComm", "batch_train_finish", "ACC_PREPARED", "batch_accumulate", "batch_update_prepare",
    "ONLINE_INT_ABS", "train_online", "batch_update", "gaussian_kernel1d", "gaussian_blur_hwc", "rowsum_filter_normalize",
    "normalize_columns", "quantile_nonzero", "to_numpy", "pair_histogram", "quantile_f32", "scaled_rowsum",
    "scaled_rowsum_f32", "MASK_BAD_LABEL", "MASK_BAD_PIXEL", "LUT_UNMAPPED", "cluster_mask", "relabel", "SEG_DTYPES",
    "SEG_F64", "SEG_ERODE", "SEGMASK_FORCE_SEARCH", "segmask_table", "segmentation_mask", "PLANE_DTYPES",
    "BLUR_MAX_RADIUS", "BLUR_SIGMA_LIMIT", "check_blur_sigma", "BLUR_MODES", "PLANE_MODE_DTYPES", "_blur_plane",
    "gaussian_blur_plane", "gaussian_blur_plane_mode", "SELECT_FILL", "SELECT_KEEP", "BIN_POSITIVE", "BIN_LEVEL",
    "BIN_LOCAL", "CCL_TILE", "_binary_plane", "_rows_plane", "_label_plane", "_like_plane", "_ld", "label_components",
    "components_select", "binarize_plane", "RIDGE_MAX_RADIUS", "RIDGE_MAX_SCALES", "ridge_sign", "object_mask",
    "PAIR_CAPACITY_MAX", "label_regions", "_label_pair", "pair_overlaps", "merge_apply", "_region_tables", "choose_merges",
    "merge_masks", "zero_by_segmentation", "AssignSumsWorkspace", "TABLES_SCRATCH_CLEAN", "_with_scratch_flag",
    "assign_sums", "assign_means", "CELLQUANT_IMAGE_DTYPES", "CELLQUANT_MODES", "CELLQUANT_FORCE_SEARCH",
    "CELLQUANT_NUC_CAPACITY", "label_keys", "_label_image", "_key_range", "cell_quantify", "REGION_FORCE_SEARCH",
    "REGION_MAX_SIDE", "CONCAVITY_DEFAULTS", "region_props", "NUCSPLIT_FORCE_SEARCH", "_split_planes", "nuclear_overlaps",
    "choose_splits", "split_nuclei_apply", "split_large_nuclei", "_smallest_double", "neighbor_thresholds", "_cell_args",
    "_check_offsets", "_cells_sorted_by_type", "neighbor_counts", "CLOSE_PAIR_MAX_SETS", "close_pair_counts",
    "NEAREST_MAX_K", "_S_ZERO", "_nearest_s_zero", "nearest_type_means", "SILHOUETTE_MAX_D", "SILHOUETTE_MAX_K",
    "_silhouette", "silhouette_samples", "silhouette_scores", "KMEANS_MAX_D", "KMEANS_MAX_K", "KMEANS_MAX_PROBLEMS",
    "_kmeans_ks", "kmeans_group_count", "kmeans_lloyd",
)
PACKAGE = "ark_analysis_amd.som_device"


def test_the_list_is_the_parents():
    assert len(PARENT_NAMES) == len(set(PARENT_NAMES)) == 64 + 23 + 47     # public, private, constants


def test_every_name_of_the_single_module_is_an_attribute_of_the_facade():
    from ark_analysis_amd import som_device
    missing = [n for n in PARENT_NAMES if not hasattr(som_device, n)]
    assert not missing, missing


def test_functions_and_classes_are_the_objects_of_their_family_module():
    from ark_analysis_amd import som_device
    checked = 0
    for name in PARENT_NAMES:
        obj = getattr(som_device, name)
        if not (inspect.isfunction(obj) or inspect.isclass(obj)):
            continue
        assert obj.__module__.startswith(PACKAGE + "."), (name, obj.__module__)
        assert getattr(importlib.import_module(obj.__module__), name) is obj, name
        checked += 1
    assert checked == 64 + 23


def test_constants_are_the_objects_of_a_family_module():
    from ark_analysis_amd import som_device
    families = [importlib.import_module(PACKAGE + "." + m)
                for m in ("_args", "som", "comm", "pixels", "planes", "cells", "spatial", "clustering")]
    for name in PARENT_NAMES:
        obj = getattr(som_device, name)
        if inspect.isfunction(obj) or inspect.isclass(obj):
            continue
        assert any(vars(m).get(name, families) is obj for m in families), name


def test_the_facade_only_imports():
    """No ``import *``, no ``__getattr__``, no definition: the facade's statements are its docstring and explicit
    relative imports."""
    import ast
    from ark_analysis_amd import som_device
    body = ast.parse(open(som_device.__file__).read()).body
    assert isinstance(body[0], ast.Expr) and isinstance(body[0].value, ast.Constant)
    for node in body[1:]:
        assert isinstance(node, ast.ImportFrom) and node.level == 1, ast.dump(node)
        assert all(a.name != "*" and a.asname is None for a in node.names)
    assert "__getattr__" not in vars(som_device)


def test_attributes_set_on_a_function_are_seen_through_the_facade():
    from ark_analysis_amd import som_device
    from ark_analysis_amd.som_device import som
    som.assign.last_workspace = marker = object()
    try:
        assert som_device.assign.last_workspace is marker
    finally:
        del som.assign.last_workspace
