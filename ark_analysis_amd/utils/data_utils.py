"""The functions of ``ark.utils.data_utils`` that sit directly behind the pixel labels
(/root/reference/src/ark/utils/data_utils.py:476-555; SURVEY.md section 8 f, rank 4): a FOV's pixel table with
SOM / meta cluster labels -> an ``[H, W]`` int16 image of cluster ids.  The relabel (label -> cluster_id) and
the scatter run on the device; path checks, the mapping table and the table read stay on the host.  Around it, the
cohort loop that saves one mask per FOV (``generate_and_save_pixel_cluster_masks``, :558-635) and ``save_fov_mask``
(:32-68).

The cell half (:70-473, :637-715): ``erode_mask`` (skimage's find_boundaries + zeroing), ``ClusterMaskData``, the
label -> cluster lookups ``relabel_segmentation`` / ``label_cells_by_cluster`` / ``map_segmentation_labels``, and the
cohort loops that save one cell or neighbourhood cluster mask per FOV.  Erosion, int32 cast, lookup and narrowing are
one pass of pxsom_segmask over the segmentation image on the device; the mapping tables are host pandas."""
import concurrent.futures
import os

import numpy as np
import pandas as pd

from .. import distributed, flowsom, image_io
from ..fov_tables import read_table
from ..host_utils import natsorted, validate_paths, verify_in_list


def generate_pixel_cluster_mask(fov, base_dir, tiff_dir, chan_file_path,
                                pixel_data_dir, cluster_mapping,
                                pixel_cluster_col='pixel_meta_cluster'):
    """For a fov, create a mask labeling each pixel with its SOM or meta cluster id.

    ``chan_file_path`` (relative to ``tiff_dir``) names a sample channel image that fixes the mask's size;
    ``cluster_mapping`` is the DataFrame that maps ``pixel_cluster_col`` values to ``cluster_id``.  Pixels the
    table does not list stay 0."""
    table_dir = os.path.join(base_dir, pixel_data_dir)
    validate_paths([tiff_dir, os.path.join(tiff_dir, chan_file_path), table_dir])
    verify_in_list(provided_cluster_col=[pixel_cluster_col],
                   valid_cluster_cols=['pixel_som_cluster', 'pixel_meta_cluster'])
    verify_in_list(provided_fov_file=[fov + '.feather'], consensus_fov_files=os.listdir(table_dir))

    sample = np.squeeze(image_io.read_image(os.path.join(tiff_dir, chan_file_path)))
    table = read_table(os.path.join(table_dir, fov + '.feather'))

    def column(name):
        return table.column(name).to_numpy()
    labels = column(pixel_cluster_col).astype(int)        # "ensure integer display and not float"

    # later rows of the mapping win for a repeated key, as in dict(zip(...))
    pairs = cluster_mapping.drop_duplicates()[[pixel_cluster_col, 'cluster_id']]
    id_mapping = dict(zip(pairs[pixel_cluster_col], pairs['cluster_id']))
    return flowsom.pixel_cluster_mask(column('row_index'), column('column_index'), labels, id_mapping,
                                      (sample.shape[0], sample.shape[1]))


def save_fov_mask(fov, data_dir, mask_data, sub_dir=None, name_suffix=''):
    """Saves a cluster mask as ``<data_dir>/[<sub_dir>/]<fov><name_suffix>.tiff``."""
    validate_paths(data_dir)
    folder = os.path.join(data_dir, sub_dir or '')
    os.makedirs(folder, exist_ok=True)
    mask = np.asarray(mask_data)
    path = os.path.join(folder, fov + name_suffix + '.tiff')
    if mask.dtype.kind in "biu" and mask.dtype not in (np.uint8, np.uint16, np.int16, np.int32):
        # dtypes the baseline TIFF writer has no sample format for (bool, uint32, int64 ... masks: the reference's tifffile
        # takes them all): the narrowest one it has that holds every value -- pixel values are unchanged
        lo, hi = (int(mask.min()), int(mask.max())) if mask.size else (0, 0)
        for dt in (np.uint8, np.uint16, np.int16, np.int32):
            if np.iinfo(dt).min <= lo and hi <= np.iinfo(dt).max:
                mask = mask.astype(dt)
                break
        else:
            raise ValueError("mask values [%d, %d] do not fit a 32-bit TIFF sample" % (lo, hi))
    elif mask.dtype == np.float64:
        as32 = mask.astype(np.float32)
        if not np.array_equal(as32.astype(np.float64), mask, equal_nan=True):
            raise ValueError("float64 mask with values float32 cannot hold: save it with a full TIFF library")
        mask = as32
    image_io.write_image(path, mask)


def generate_and_save_pixel_cluster_masks(fovs, base_dir, save_dir, tiff_dir, chan_file, pixel_data_dir,
                                          cluster_id_to_name_path, pixel_cluster_col='pixel_meta_cluster',
                                          sub_dir=None, name_suffix=''):
    """One cluster-id mask per FOV, saved under ``save_dir``.  The cluster -> name table at
    ``cluster_id_to_name_path`` (the remapping GUI's output) gets a ``cluster_id`` column -- 1, 2, ... over the
    distinct ``pixel_cluster_col`` values in ascending order -- and is rewritten in place; those ids are what the
    masks hold.  ``chan_file``: a channel image inside every FOV folder, for the mask's size."""
    # under a process group (torchrun) rank 0 rewrites the table, the FOVs are dealt out by rank
    rank, world = distributed.init_from_env()
    mapping = None
    if rank == 0:
        names = pd.read_csv(cluster_id_to_name_path)
        ids = names[[pixel_cluster_col]].drop_duplicates().sort_values(by=[pixel_cluster_col])
        ids["cluster_id"] = list(range(1, len(ids) + 1))
        mapping = names.drop(columns="cluster_id", errors="ignore").merge(ids, on=[pixel_cluster_col], how="left")
        mapping.to_csv(cluster_id_to_name_path, index=False)
    mapping = distributed.broadcast_object(mapping, 0)
    for fov in distributed.shard(fovs, rank, world):
        mask = generate_pixel_cluster_mask(fov=fov, base_dir=base_dir, tiff_dir=tiff_dir,
                                           chan_file_path=os.path.join(fov, chan_file), pixel_data_dir=pixel_data_dir,
                                           cluster_mapping=mapping, pixel_cluster_col=pixel_cluster_col)
        save_fov_mask(fov, data_dir=save_dir, mask_data=mask, sub_dir=sub_dir, name_suffix=name_suffix)
    distributed.barrier()


# ---- cell cluster masks ---------------------------------------------------------------------------------------------
# The reference's column names (ark.settings): FOV_ID, CELL_LABEL, CELL_TYPE, KMEANS_CLUSTER
_FOV_ID, _CELL_LABEL, _CELL_TYPE, _KMEANS_CLUSTER = "fov", "label", "cell_meta_cluster", "kmeans_neighborhood"
_DEVICE_DTYPES = tuple(np.dtype(t) for t in (np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64))


def _as_array(label_map) -> np.ndarray:
    """A label map as an ndarray: numpy arrays, or anything with ``.values`` (an xarray DataArray)."""
    if isinstance(label_map, np.ndarray):
        return label_map
    return np.asarray(getattr(label_map, "values", label_map))


def _table(keys, values, float_values):
    """(keys, values) pairs as the sorted int32 key table of pxsom_segmask: keys wrap to int32 as numba's int32-keyed
    dict stores them, and a later pair wins over an earlier one with the same key."""
    keys = np.asarray(keys).astype(np.int64).astype(np.int32)
    values = np.asarray(values, dtype=np.float64 if float_values else None)
    if not float_values:
        values = values.astype(np.int64).astype(np.int32)
    if keys.size == 0:
        return keys, values
    uniq, first_from_end = np.unique(keys[::-1], return_index=True)
    return uniq, values[::-1][first_from_end]


def _segmask_device(seg, erode=None, connectivity=1, background=0, table=None, unassigned=0, out_dtype=None):
    """pxsom_segmask on a 2-D host label image of a device dtype -> host array of ``out_dtype`` (default: seg's).
    ``table``: (sorted int32 keys, int32 or float64 values) or None.  The one device entry point of the cell masks (the
    CPU tests swap it for the numpy statement of the same contract)."""
    import torch
    from .. import _capi, som_device
    dev = _capi.require_gpu()
    seg = np.ascontiguousarray(seg)
    out_dtype = np.dtype(out_dtype or seg.dtype)
    t = torch.from_numpy(seg if seg.flags.writeable else seg.copy()).to(dev, non_blocking=False)
    dev_table = None
    if table is not None:
        dev_table = som_device.segmask_table(table[0], table[1], dev, float_values=out_dtype == np.float64)
    torch_out = {np.dtype(np.float64): torch.float64, np.dtype(np.int16): torch.int16,
                 np.dtype(np.int32): torch.int32}.get(out_dtype, t.dtype)
    out = som_device.segmentation_mask(t, erode=erode, connectivity=connectivity, background=background,
                                       table=dev_table, unassigned=unassigned, out_dtype=torch_out)
    return out.cpu().numpy()


def _relabel(labels: np.ndarray, table, unassigned, out_dtype, erode=None, connectivity=1, background=0) -> np.ndarray:
    """Erosion (optional) + lookup of a label image of any shape whose non-singleton axes are at most two; the result
    keeps the image's shape.  Device dtypes go as they are; any other dtype is cast to int32 on the host first (what
    the reference does to every label image before its lookup)."""
    labels = _as_array(labels)
    if labels.dtype not in _DEVICE_DTYPES:
        if erode is not None:
            labels = erode_mask(labels, connectivity=connectivity, mode=erode, background=background)
            erode = None
        labels = labels.astype(np.int32)
    plane = np.squeeze(labels)
    if plane.ndim > 2:
        raise NotImplementedError("label stacks deeper than one plane are not supported")
    out_dtype = np.dtype(out_dtype)
    dev_out = out_dtype if out_dtype in (np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.float64)) else (
        np.dtype(np.float64) if out_dtype.kind == "f" else np.dtype(np.int32))
    res = _segmask_device(np.atleast_2d(plane), erode, connectivity, background, table, unassigned, dev_out)
    return res.reshape(labels.shape).astype(out_dtype, copy=False)


def _find_boundaries_host(seg, connectivity, mode, background):
    """find_boundaries on the host for the dtypes the device pass does not take (bool, float, int8, uint64): the
    same definition, dilation != erosion of scipy.ndimage under its reflect border, "inner" excluding background."""
    import scipy.ndimage as ndi
    img = seg.astype(np.uint8) if seg.dtype == bool else seg
    fp = ndi.generate_binary_structure(img.ndim, connectivity)
    edge = ndi.grey_dilation(img, footprint=fp) != ndi.grey_erosion(img, footprint=fp)
    if mode == "inner":
        edge &= img != background
    return edge


def erode_mask(seg_mask, **kwargs) -> np.ndarray:
    """Zeroes the border pixels of every label: ``skimage.segmentation.find_boundaries(seg_mask, **kwargs)`` (keywords
    ``connectivity`` = 1, ``mode`` = "thick" or "inner", ``background`` = 0), then ``np.where(edges == 0, seg_mask, 0)``.
    Integer images of uint8 / int16 / uint16 / int32 / uint32 / int64 take the device pass; other dtypes (bool, float)
    are eroded on the host with scipy.ndimage by the same definition.  Singleton axes (``[H, W, 1]``) are kept."""
    connectivity = kwargs.pop("connectivity", 1)
    mode = kwargs.pop("mode", "thick")
    background = kwargs.pop("background", 0)
    kwargs.pop("label_img", None)
    if kwargs:
        raise TypeError("erode_mask: unexpected keyword arguments %s" % sorted(kwargs))
    if mode not in ("thick", "inner"):
        raise NotImplementedError("find_boundaries mode %r: only 'thick' and 'inner' are implemented" % (mode,))
    seg = _as_array(seg_mask)
    if seg.dtype in _DEVICE_DTYPES and seg.size:
        plane = np.squeeze(seg)
        if plane.ndim > 2:
            raise NotImplementedError("label stacks deeper than one plane are not supported")
        out = _segmask_device(np.atleast_2d(plane), mode, max(int(connectivity), 1), int(background))
        return out.reshape(seg.shape)
    edges = _find_boundaries_host(seg, connectivity, mode, background)
    return np.where(edges == 0, seg, 0)


class ClusterMaskData:
    """The cohort's segmentation label -> cluster id table.  Cluster ids 1, 2, ... number the distinct values of
    ``cluster_col`` in ascending order (ints or strings: ``cluster_name_id``); every FOV gets a label 0 -> cluster 0
    row; ``mapping`` is sorted by (fov, label), stable, so for a (fov, label) listed twice the later row wins in the
    lookup, and a table row with label 0 loses to the added background row.  ``unassigned_id`` = ``n_clusters`` + 1
    marks cells the table does not list."""

    def __init__(self, data: pd.DataFrame, fov_col: str, label_col: str, cluster_col: str) -> None:
        self.fov_column = fov_col
        self.label_column = label_col
        self.cluster_column = cluster_col
        self.cluster_id_column = "cluster_id"
        table = data[[fov_col, label_col, cluster_col]].copy()

        names = pd.DataFrame({cluster_col: table[cluster_col].unique()})
        names = names.sort_values(by=cluster_col).reset_index(drop=True)
        names[self.cluster_id_column] = (names.index + 1).astype(np.int32)
        self.cluster_name_id = names

        types = {fov_col: str, label_col: np.int32, self.cluster_id_column: np.int32}
        table = table.merge(right=names, on=cluster_col).astype(types)
        self.unique_fovs = natsorted(table[fov_col].unique().tolist())
        top = table[self.cluster_id_column].max()
        self.unassigned_id = np.int32(top + 1)
        self.n_clusters = top

        zeros = np.zeros(len(self.unique_fovs), dtype=np.int64)
        background = pd.DataFrame({fov_col: self.unique_fovs, label_col: zeros, cluster_col: zeros,
                                   self.cluster_id_column: zeros})
        table = pd.concat([table, background]).astype(types)
        self.mapping = table.sort_values(by=[fov_col, label_col])

    def fov_mapping(self, fov: str) -> pd.DataFrame:
        """The rows of one FOV (ValueError for a FOV the table lacks)."""
        verify_in_list(requested_fov=[fov], all_fovs=self.unique_fovs)
        return self.mapping[self.mapping[self.fov_column] == fov].reset_index(drop=True)

    @property
    def cluster_names(self) -> list:
        return self.cluster_name_id[self.cluster_column].tolist()


def _fov_table(fov, cmd):
    verify_in_list(fov_name=[fov], all_data_fovs=cmd.unique_fovs)
    rows = cmd.fov_mapping(fov=fov)
    return _table(rows[cmd.label_column].to_numpy(), rows[cmd.cluster_id_column].to_numpy(), False)


def label_cells_by_cluster(fov: str, cmd: ClusterMaskData, label_map) -> np.ndarray:
    """The FOV's label image with every cell replaced by its cluster id (``cmd.unassigned_id`` for cells the table
    lacks, 0 for background), as int16: ids are found for the int32 cast of each label and narrowed the way
    ``astype(np.int16)`` narrows them.  ``label_map``: an array or anything with ``.values``; singleton axes go."""
    table = _fov_table(fov, cmd)
    labels = np.squeeze(_as_array(label_map))
    return _relabel(labels, table, int(cmd.unassigned_id), np.int16)


def relabel_segmentation(mapping: dict, unassigned_id, labeled_image: np.ndarray, _dtype=np.float64) -> np.ndarray:
    """``mapping.get(label, unassigned_id)`` for every pixel of a 2-D label image, as ``_dtype``.  ``mapping`` is a plain
    dict (the reference's numba dict has int32 keys: keys and labels are compared after their int32 cast; values are
    int32 for an integer ``_dtype``, float64 for a float one)."""
    float_values = np.dtype(_dtype).kind == "f"
    table = _table(list(mapping.keys()), list(mapping.values()), float_values)
    return _relabel(labeled_image, table, unassigned_id, _dtype)


def map_segmentation_labels(labels, values, label_map, unassigned_id: float = 0) -> np.ndarray:
    """A float64 image holding, for every pixel, the value of its cell (``labels[i]`` -> ``values[i]``; the last of a
    repeated label wins) or ``unassigned_id``.  NaN and +-inf in a ``values`` Series become 0 (an ndarray is taken as
    it is)."""
    if isinstance(labels, pd.Series):
        labels = labels.to_numpy(dtype=np.int32)
    if isinstance(values, pd.Series):
        values = values.to_numpy(dtype=np.float64)
        values = np.where(np.isfinite(values), values, 0.0)
    labels, values = np.ravel(labels), np.ravel(np.asarray(values, dtype=np.float64))
    n = min(labels.size, values.size)       # pairs as zip() forms them
    table = _table(labels[:n], values[:n], True)
    return _relabel(np.squeeze(_as_array(label_map)), table, float(unassigned_id), np.float64)


def _segmentation_path(seg_dir, fov, seg_suffix):
    path = os.path.join(seg_dir, fov + seg_suffix)
    validate_paths([seg_dir])
    if not os.path.isfile(path):        # what the reference's image loader raises for a file it cannot find
        raise ValueError("Invalid value for %s. %s is not a valid file." % (fov + seg_suffix, path))
    return path


def _read_segmentation(seg_dir, fov, seg_suffix) -> np.ndarray:
    return image_io.read_image(_segmentation_path(seg_dir, fov, seg_suffix))


def _cluster_mask_from(fov, seg, cmd, erode) -> np.ndarray:
    table = _fov_table(fov, cmd)
    if erode:   # erode_mask(connectivity=2, mode="thick", background=0), then label_cells_by_cluster: one device pass
        return _relabel(seg, table, int(cmd.unassigned_id), np.int16, erode="thick", connectivity=2)
    return _relabel(seg, table, int(cmd.unassigned_id), np.int16)


def generate_cluster_mask(fov: str, seg_dir, cmd: ClusterMaskData, seg_suffix: str = "_whole_cell.tiff",
                          erode: bool = True, **kwargs) -> np.ndarray:
    """The FOV's int16 cell cluster mask: its segmentation ``<seg_dir>/<fov><seg_suffix>``, borders eroded (8-neighbour
    "thick" boundaries) unless ``erode`` is False, each cell replaced by its cluster id (label_cells_by_cluster)."""
    validate_paths([seg_dir])
    return _cluster_mask_from(fov, _read_segmentation(seg_dir, fov, seg_suffix), cmd, erode)


def _save_masks(fovs, seg_dir, seg_suffix, make_mask, save_dir, sub_dir, name_suffix):
    """make_mask(fov, seg) for this rank's share of ``fovs``, each saved with save_fov_mask.  The next FOV's
    segmentation is read by a helper thread while the current one is on the device."""
    validate_paths([seg_dir])
    mine = distributed.shard(fovs)
    with concurrent.futures.ThreadPoolExecutor(max_workers=1) as reader:
        ahead = reader.submit(_read_segmentation, seg_dir, mine[0], seg_suffix) if mine else None
        for i, fov in enumerate(mine):
            seg = ahead.result()
            ahead = reader.submit(_read_segmentation, seg_dir, mine[i + 1], seg_suffix) if i + 1 < len(mine) else None
            save_fov_mask(fov, data_dir=save_dir, mask_data=make_mask(fov, seg), sub_dir=sub_dir,
                          name_suffix=name_suffix)


def generate_and_save_cell_cluster_masks(fovs, save_dir, seg_dir, cell_data: pd.DataFrame, cluster_id_to_name_path,
                                         fov_col: str = _FOV_ID, label_col: str = _CELL_LABEL,
                                         cell_cluster_col: str = _CELL_TYPE, seg_suffix: str = "_whole_cell.tiff",
                                         sub_dir=None, name_suffix: str = ""):
    """One int16 cell cluster mask per FOV (generate_cluster_mask, eroded), saved as
    ``<save_dir>/[<sub_dir>/]<fov><name_suffix>.tiff``.  The cluster -> name table at ``cluster_id_to_name_path`` (the
    remapping GUI's CSV) is rewritten with the ``cluster_id`` column the masks hold.  Under a process group (torchrun)
    rank 0 builds the mapping and rewrites the CSV, every rank gets the mapping, and the FOVs are dealt out by rank."""
    distributed.init_from_env()

    def mapping_and_csv():
        cmd = ClusterMaskData(data=cell_data, fov_col=fov_col, label_col=label_col, cluster_col=cell_cluster_col)
        ids = cmd.mapping.filter([cmd.cluster_column, cmd.cluster_id_column]).drop_duplicates()
        names = pd.read_csv(cluster_id_to_name_path).drop(columns="cluster_id", errors="ignore")
        names.merge(ids, on=[cmd.cluster_column], how="left").to_csv(cluster_id_to_name_path, index=False)
        return cmd
    cmd = distributed.on_rank0(mapping_and_csv)   # an error on rank 0 is raised on every rank
    _save_masks(fovs, seg_dir, seg_suffix, lambda fov, seg: _cluster_mask_from(fov, seg, cmd, True),
                save_dir, sub_dir, name_suffix)
    distributed.barrier()


def generate_and_save_neighborhood_cluster_masks(fovs, save_dir, seg_dir, neighborhood_data: pd.DataFrame,
                                                 fov_col: str = _FOV_ID, label_col: str = _CELL_LABEL,
                                                 cluster_col: str = _KMEANS_CLUSTER, seg_suffix: str = "_whole_cell.tiff",
                                                 xr_channel_name="label", sub_dir=None, name_suffix: str = ""):
    """One int16 neighbourhood cluster mask per FOV: label_cells_by_cluster keyed by ``cluster_col`` (the k-means
    neighbourhood), without erosion, saved as generate_and_save_cell_cluster_masks saves.  ``xr_channel_name`` only
    names the channel of the reference's label array; it does not change the mask."""
    distributed.init_from_env()
    cmd = distributed.on_rank0(lambda: ClusterMaskData(data=neighborhood_data, fov_col=fov_col, label_col=label_col,
                                                       cluster_col=cluster_col))
    _save_masks(fovs, seg_dir, seg_suffix, lambda fov, seg: _cluster_mask_from(fov, seg, cmd, False),
                save_dir, sub_dir, name_suffix)
    distributed.barrier()
