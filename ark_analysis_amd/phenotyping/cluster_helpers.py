"""SOM cluster objects -- the classes ``ark.phenotyping.cluster_helpers`` exposes for the Pixie SOM steps
(/root/reference/src/ark/phenotyping/cluster_helpers.py:52-416), re-implemented over the gfx950 kernels.

Public surface kept so notebooks and the reference's tests run unchanged: class names, constructor
arguments and defaults, the attributes callers read (``weights``, ``weights_path``, ``columns``,
``norm_data``, ``train_data``, ``cell_data``, ``fovs``, ``som_clusters_seen``), the warning texts and the
on-disk weights format (feather, one row per node, row k <-> label k + 1).  ``pyFlowSOM.som`` /
``pyFlowSOM.map_data_to_nodes`` are :func:`ark_analysis_amd.flowsom.som` /
:func:`~ark_analysis_amd.flowsom.map_data_to_nodes`.

Objects hold host state only (pandas / numpy) and therefore pickle; device buffers live for one call.

Beyond the reference (keyword-only, defaults = the reference's behaviour): ``train_mode="batch"`` with
``batch_steps`` trains with the data-parallel batch rule (``flowsom.som_batch``) instead of the sequential
online rule.  Under ``torchrun`` (``ark_analysis_amd.distributed.init_from_env``) a batch-mode object loads
only its rank's share of the training tables, the per-step statistics are all-reduced over RCCL, and rank 0
writes the codebook file; an online-mode object is trained by rank 0 alone and broadcast (the online rule is
sequential: replicas only).

Deliberate differences:
* training tables are concatenated in natural-sorted FOV order -- the reference takes ``os.listdir``
  order (:211-215), which is file-system dependent, and the presentation order is an input of the SOM;
* rows are handed to the BMU search in positional blocks (the reference slices by index label,
  :154-156, which selects the same rows for the RangeIndex every table reader produces).
"""
import os
import pathlib
import warnings
from abc import ABC, abstractmethod
from typing import Iterator, List, Optional, Tuple

import numpy as np
import pandas as pd

from .. import distributed, flowsom
from ..fov_tables import FovTableDir, read_dataframe, write_dataframe  # noqa: F401  (re-exported)
from ..host_utils import validate_paths, verify_in_list


def _capi_limits() -> Tuple[int, int]:
    """(max feature columns, max nodes) of the kernels: PXSOM_MAX_CHANNELS, PXSOM_MAX_NODES."""
    from .. import _capi
    return _capi.MAX_CHANNELS, _capi.MAX_NODES


def _row_blocks(n_rows: int, block: int) -> Iterator[Tuple[int, int]]:
    """[start, stop) bounds of consecutive blocks of at most ``block`` rows."""
    start = 0
    while start < n_rows:
        yield start, min(start + block, n_rows)
        start += block


def _as_f64_matrix(frame: pd.DataFrame) -> np.ndarray:
    return np.ascontiguousarray(frame.to_numpy(dtype=np.float64))


class PixieSOMCluster(ABC):
    """What pixel and cell SOMs share: the grid, the schedule, the codebook file and the two kernel
    calls (reference base class: cluster_helpers.py:52-163)."""

    #: words of the "already trained" / "retraining" warnings; the subclasses fill them in
    _subject = ("SOM", "columns")

    @abstractmethod
    def __init__(self, weights_path: pathlib.Path, columns: List[str], num_passes: int = 1,
                 xdim: int = 10, ydim: int = 10, lr_start: float = 0.05, lr_end: float = 0.01,
                 seed=42, *, train_mode: str = "online", batch_steps=None, distf: int = 2):
        if train_mode not in ("online", "batch"):
            raise ValueError("train_mode must be 'online' (the reference's rule) or 'batch', got %r" % (train_mode,))
        # FlowSOM's distance code of the BMU search, in training AND labelling (1 Manhattan, 2 Euclidean, 3 Chebyshev, 4 cosine;
        # parity with pyFlowSOM unpinned).  The weights file does not record it: this object carries it from one to the other.
        self.distf = flowsom._check_distf(distf)
        from ..schedule import resolve
        resolve(batch_steps)     # ValueError("batch_steps ...") for anything but a positive int / "two-phase" / a schedule
        self.train_mode, self.batch_steps = train_mode, batch_steps
        # limits of the gfx950 kernels (include/pxsom.h): said here, where the user chose the shape, rather than as
        # a kernel status code in the middle of a run
        if len(columns) > _capi_limits()[0] or int(xdim) * int(ydim) > _capi_limits()[1]:
            raise ValueError("this build's SOM kernels take at most %d feature columns and %d nodes; got %d columns "
                             "on a %d x %d grid" % (_capi_limits() + (len(columns), xdim, ydim)))
        self.weights_path = weights_path
        self.columns = columns
        self.xdim, self.ydim = xdim, ydim
        self.lr_start, self.lr_end = lr_start, lr_end
        self.num_passes = num_passes
        self.seed = seed
        # a codebook written by an earlier session is picked up again
        self.weights: Optional[pd.DataFrame] = read_dataframe(weights_path) \
            if os.path.exists(weights_path) else None

    @abstractmethod
    def normalize_data(self) -> pd.DataFrame:
        """Scaling of the input columns; each subclass has its own rule."""

    # ---- training ---------------------------------------------------------------------------
    def _needs_training(self, overwrite: bool) -> bool:
        """The reference's three-way decision with its three warnings (:250-268, :374-393)."""
        kind, what = self._subject
        if overwrite:
            warnings.warn("Overwrite flag set, retraining SOM")
            return True
        if self.weights is None:
            return True
        if set(self.weights.columns.values) == set(self.columns):
            warnings.warn("%s SOM already trained on specified %s" % (kind, what))
            return False
        warnings.warn("New %s specified, retraining" % what)
        return True

    def train_som(self, data: pd.DataFrame):
        """Fit the xdim x ydim codebook on the rows of ``data`` (``num_passes`` passes, learning rate
        ``lr_start`` -> ``lr_end``; FlowSOM online rule, or the batch rule in ``train_mode="batch"``) and store it
        at ``weights_path``.  With a process group: see the module docstring."""
        rank, world = distributed.context()
        args = dict(xdim=self.xdim, ydim=self.ydim, rlen=self.num_passes,
                    alpha_range=(self.lr_start, self.lr_end), seed=self.seed)
        if self.train_mode == "batch":
            codebook = flowsom.som_batch(data=_as_f64_matrix(data), batch_steps=self.batch_steps, distf=self.distf, **args)
        else:
            # rank 0 trains, the others receive the codebook -- or rank 0's exception (never a wait without end)
            codebook = distributed.on_rank0(lambda: flowsom.som(data=_as_f64_matrix(data), distf=self.distf, **args))
        nodes = self.xdim * self.ydim
        self.weights = pd.DataFrame(np.asarray(codebook).reshape(nodes, -1), columns=data.columns.values)
        if rank == 0:
            write_dataframe(self.weights, self.weights_path, compression="uncompressed")
        distributed.barrier()   # nobody goes on to read a half-written codebook file

    # ---- assignment -------------------------------------------------------------------------
    def generate_som_clusters(self, external_data: pd.DataFrame,
                              num_parallel_obs: int = 1000000) -> np.ndarray:
        """1-based best-matching-unit label of every row of ``external_data`` (first minimum wins),
        searched in blocks of ``num_parallel_obs`` rows."""
        if num_parallel_obs <= 0:
            raise ValueError("num_parallel_obs specified needs to be greater than 0")

        trained_on = self.weights.columns.values
        verify_in_list(weights_cols=trained_on, external_data_cols=external_data.columns.values)

        codebook = _as_f64_matrix(self.weights)
        features = external_data[list(trained_on)]  # also puts the columns in codebook order
        found = [flowsom.map_data_to_nodes(codebook, _as_f64_matrix(features.iloc[lo:hi]), distf=self.distf)[0]
                 for lo, hi in _row_blocks(len(external_data), num_parallel_obs)]
        # an image without retained pixels gives an empty (float) vector, like the reference
        return np.concatenate(found) if found else np.empty(0)


class PixelSOMCluster(PixieSOMCluster):
    """Pixel SOM: trains on the sub-sampled tables of ``pixel_subset_folder``, values divided by the
    per-channel 99.9 % row of ``norm_vals_path`` (reference: cluster_helpers.py:166-301)."""

    _subject = ("Pixel", "markers")

    def __init__(self, pixel_subset_folder: pathlib.Path, norm_vals_path: pathlib.Path,
                 weights_path: pathlib.Path, fovs: List[str], columns: List[str],
                 num_passes: int = 1, xdim: int = 10, ydim: int = 10,
                 lr_start: float = 0.05, lr_end: float = 0.01, seed=42, *,
                 train_mode: str = "online", batch_steps=None, distf: int = 2):
        super().__init__(weights_path, columns, num_passes, xdim, ydim, lr_start, lr_end, seed,
                         train_mode=train_mode, batch_steps=batch_steps, distf=distf)
        validate_paths([norm_vals_path, pixel_subset_folder])

        self.fovs = fovs
        self.norm_data = read_dataframe(norm_vals_path)
        self.som_clusters_seen = set()

        wanted = set(fovs)
        subset = FovTableDir(pixel_subset_folder)
        mine = [fov for fov in subset.fovs() if fov in wanted]
        if self.train_mode == "batch":
            # data-parallel training: every rank holds its share of the FOVs (all of them without a process group)
            mine = distributed.shard(mine) or mine[:0]
        parts = [subset.load(fov) for fov in mine]
        if not parts:   # more ranks than FOVs: an empty table with the right columns
            parts = [subset.load(subset.fovs()[0]).iloc[:0]]
        # the training matrix is only ever used normalised
        self.train_data = self.normalize_data(pd.concat(parts))

    def normalize_data(self, external_data: pd.DataFrame) -> pd.DataFrame:
        """Copy of ``external_data`` with every channel of ``norm_data`` divided by its norm value."""
        channels = self.norm_data.columns.values
        verify_in_list(norm_data_cols=channels, external_data_cols=external_data.columns.values)

        scaled = external_data.copy()
        divisors = self.norm_data.iloc[0].to_numpy(dtype=np.float64)
        scaled[channels] = scaled[channels].to_numpy() / divisors   # IEEE division per element
        return scaled

    def train_som(self, overwrite=False):
        if self._needs_training(overwrite):
            super().train_som(self.train_data[self.columns])

    def assign_som_clusters(self, external_data: pd.DataFrame, normalize_data: bool = True,
                            num_parallel_pixels: int = 1000000) -> pd.DataFrame:
        """``external_data`` (normalised unless told otherwise) plus a ``pixel_som_cluster`` column;
        the labels met are remembered in ``som_clusters_seen``."""
        table = self.normalize_data(external_data) if normalize_data else external_data.copy()
        labels = self.generate_som_clusters(table, num_parallel_obs=num_parallel_pixels)
        table["pixel_som_cluster"] = labels
        self.som_clusters_seen.update(np.unique(labels).tolist())
        return table


class CellSOMCluster(PixieSOMCluster):
    """Cell SOM over a cell x feature table held in memory; features are scaled by their own 99.9 %
    quantile of non-zero values (reference: cluster_helpers.py:304-416)."""

    _subject = ("Cell", "columns")

    def __init__(self, cell_data: pd.DataFrame, weights_path: pathlib.Path,
                 fovs: List[str], columns: List[str], num_passes: int = 1,
                 xdim: int = 10, ydim: int = 10, lr_start: float = 0.05, lr_end: float = 0.01,
                 seed=42, normalize=True, *, train_mode: str = "online", batch_steps=None, distf: int = 2):
        super().__init__(weights_path, columns, num_passes, xdim, ydim, lr_start, lr_end, seed,
                         train_mode=train_mode, batch_steps=batch_steps, distf=distf)
        self.fovs = fovs
        in_cohort = cell_data["fov"].isin(fovs)
        self.cell_data = cell_data[in_cohort].reset_index(drop=True)
        if normalize:
            self.normalize_data()

    def normalize_data(self):
        """In place: each training column divided by the 0.999 quantile of its non-zero entries."""
        block = self.cell_data[self.columns]
        caps = block.where(block != 0).quantile(q=0.999, axis=0)   # zeros -> NaN -> ignored
        self.cell_data[self.columns] = block.div(caps)

    def train_som(self, overwrite=False):
        if self._needs_training(overwrite):
            rows = self.cell_data[self.columns]
            if self.train_mode == "batch":
                rank, world = distributed.context()
                rows = rows.iloc[rank::world]     # every rank holds the whole table: a strided share each
            super().train_som(rows)

    def assign_som_clusters(self, num_parallel_cells=1000000) -> pd.DataFrame:
        """Adds ``cell_som_cluster`` to ``cell_data`` and returns the table.  With a process group every rank
        labels a contiguous block of the cells and the blocks are gathered."""
        rank, world = distributed.context()
        table = self.cell_data[self.columns]
        if world > 1:
            bounds = np.linspace(0, len(table), world + 1).astype(np.int64)
            part = self.generate_som_clusters(table.iloc[bounds[rank]:bounds[rank + 1]],
                                              num_parallel_obs=num_parallel_cells)
            blocks = [b for b in distributed.allgather_objects(part) if len(b)]
            labels = np.concatenate(blocks) if blocks else np.empty(0)
        else:
            labels = self.generate_som_clusters(table, num_parallel_obs=num_parallel_cells)
        self.cell_data["cell_som_cluster"] = labels
        return self.cell_data


# ---- consensus (meta) clustering of the SOM clusters ----------------------------------------------------------
# reference: cluster_helpers.py:19-49 (verify_unique_meta_clusters), :437-573 (ConsensusCluster, after
# github.com/ZigaSajovic/Consensus_Clustering; Monti et al. 2003), :575-682 (PixieConsensusCluster).
# A K x C table (K = xdim*ydim SOM clusters): host work by design (SURVEY.md section 8 f rank 4: "Ward on K x C
# stays on CPU").  What reaches the per-pixel data is a K-entry lookup table (pixel_meta_clustering.py).

def verify_unique_meta_clusters(pixie_remapped_data: pd.DataFrame, meta_cluster_type: str):
    """Every base meta cluster must carry its own renamed meta cluster: raises ``ValueError`` naming the renamed
    values that are shared by several ``{pixel,cell}_meta_cluster`` ids."""
    verify_in_list(specified_meta_cluster=meta_cluster_type, acceptable_meta_clusters=["pixel", "cell"])
    base, renamed = "%s_meta_cluster" % meta_cluster_type, "%s_meta_cluster_rename" % meta_cluster_type
    pairs = pixie_remapped_data[[base, renamed]].drop_duplicates()
    shared = pairs[pairs.duplicated(renamed, keep=False)][renamed].unique().tolist()
    if shared:
        raise ValueError("Duplicate renamed %s meta cluster values found: %s, "
                         "please re-run remapping GUI to resolve naming conflicts" % (meta_cluster_type, str(shared)))


class ConsensusCluster:
    """Consensus clustering over resamples (Monti et al. 2003): for every cluster count k in [L, K), H resamples of
    ``resample_proportion`` of the rows are clustered, ``Mk[k - L][a, b]`` is the fraction of the resamples holding
    both a and b that put them in one cluster; ``Ak`` is the area under the CDF of each consensus matrix,
    ``deltaK`` its relative change, ``bestK`` the k chosen from it.  ``cluster`` is a class taking ``n_clusters``
    with a ``fit_predict`` method.

    ark only ever builds it with L == K == max_k (reference :617-623), where no resampling takes place at all:
    ``Mk`` is an empty stack, ``bestK`` = L, and ``predict_data`` is one clustering of the data itself.  That
    configuration is what the fixtures pin.  For L < K this class computes the consensus matrices symmetrically
    (co-clustering counts over co-sampling counts); the reference's loop files a pair under [a, b] or [b, a]
    depending on sort order in one count and on sampling order in the other, which this build does not imitate."""

    def __init__(self, cluster, L: int, K: int, H: int, resample_proportion: float = 0.5):
        assert 0 <= resample_proportion <= 1, "proportion has to be between 0 and 1"
        self.cluster_ = cluster
        self.resample_proportion_ = resample_proportion
        self.L_, self.K_, self.H_ = L, K, H
        self.Mk = None
        self.Ak = None
        self.deltaK = None
        self.bestK = None

    def _internal_resample(self, data: np.ndarray, proportion: float):
        chosen = np.random.choice(range(data.shape[0]), size=int(data.shape[0] * proportion), replace=False)
        return chosen, data[chosen, :]

    def fit(self, data, verbose: bool = False):
        n = data.shape[0]
        values = np.asarray(data)
        self.Mk = np.zeros((self.K_ - self.L_, n, n))
        for k in range(self.L_, self.K_):
            together = np.zeros((n, n))      # times a and b shared a cluster
            sampled = np.zeros((n, n))       # times a and b were both drawn
            for h in range(self.H_):
                if verbose:
                    print("At k = %d, resampling h = %d" % (k, h))
                chosen, rows = self._internal_resample(values, self.resample_proportion_)
                found = np.asarray(self.cluster_(n_clusters=k).fit_predict(rows))
                member = np.zeros((n, k))
                member[chosen, found] = 1.0
                together += member @ member.T
                drawn = np.zeros(n)
                drawn[chosen] = 1.0
                sampled += np.outer(drawn, drawn)
            consensus = together / (sampled + 1e-8)
            np.fill_diagonal(consensus, 1)   # always with self
            self.Mk[k - self.L_] = consensus
        self.Ak = np.zeros(self.K_ - self.L_)
        for i, m in enumerate(self.Mk):
            hist, bins = np.histogram(m.ravel(), density=True)
            self.Ak[i] = float(np.sum(np.cumsum(hist) * np.diff(bins)))
        self.deltaK = np.array([(nxt - cur) / cur if k > 2 else cur
                                for nxt, cur, k in zip(self.Ak[1:], self.Ak[:-1], range(self.L_, self.K_ - 1))])
        self.bestK = int(np.argmax(self.deltaK)) + self.L_ if self.deltaK.size > 0 else self.L_

    def predict(self):
        assert self.Mk is not None, "First run fit"
        return self.cluster_(n_clusters=self.bestK).fit_predict(1 - self.Mk[self.bestK - self.L_])

    def predict_data(self, data):
        assert self.Mk is not None, "First run fit"
        return self.cluster_(n_clusters=self.bestK).fit_predict(data)


class PixieConsensusCluster:
    """The meta-clustering step of Pixie: z-score and cap the per-SOM-cluster average table, cluster its rows into
    ``max_k`` groups (agglomerative, Ward linkage -- scikit-learn's ``AgglomerativeClustering`` defaults, as in the
    reference) and keep the SOM cluster -> meta cluster table in ``mapping`` (1-based meta ids)."""

    def __init__(self, cluster_type: str, input_file: pathlib.Path, columns: List[str], max_k: int = 20,
                 cap: float = 3):
        from sklearn.cluster import AgglomerativeClustering
        verify_in_list(provided_cluster_type=cluster_type, supported_cluster_types=['pixel', 'cell'])
        validate_paths([input_file])
        self.cluster_type = cluster_type
        self.som_col = '%s_som_cluster' % cluster_type
        self.meta_col = '%s_meta_cluster' % cluster_type
        self.input_file = input_file
        self.input_data = pd.read_csv(input_file)
        self.columns = columns
        self.max_k = max_k
        self.cap = cap
        # H = 10 / 0.8 mirror ConsensusClusterPlus' reps / pItem defaults; with L == K they never come into play
        self.cc = ConsensusCluster(cluster=AgglomerativeClustering, L=max_k, K=max_k, H=10, resample_proportion=0.8)
        self.mapping = None

    def scale_data(self):
        """Column-wise z-score (population standard deviation), then clip to [-cap, cap]."""
        from scipy.stats import zscore
        scaled = self.input_data[self.columns].apply(zscore)
        self.input_data[self.columns] = scaled.clip(lower=-self.cap, upper=self.cap)

    def run_consensus_clustering(self):
        self.cc.fit(self.input_data[self.columns])

    def generate_som_to_meta_map(self):
        """``mapping``: one row per SOM cluster of the input table, columns [som_col, meta_col], integers."""
        self.input_data[self.meta_col] = self.cc.predict_data(self.input_data[self.columns])
        self.mapping = self.input_data[[self.som_col, self.meta_col]].copy().astype(int)
        self.mapping.loc[:, self.meta_col] += 1      # clusters are 1-based everywhere else

    def save_som_to_meta_map(self, save_path: pathlib.Path):
        write_dataframe(self.mapping, save_path)

    def lookup_table(self) -> np.ndarray:
        """``mapping`` as a dense table: ``lut[som_label]`` = meta id, ``-1`` where the mapping has no entry (what
        ``Series.map`` turns into NaN).  This is the form the per-pixel pass applies."""
        som = self.mapping[self.som_col].to_numpy(dtype=np.int64)
        lut = np.full(int(som.max()) + 1 if som.size and som.max() >= 0 else 1, -1, dtype=np.int64)
        lut[som] = self.mapping[self.meta_col].to_numpy(dtype=np.int64)   # later rows win, as dict(zip()) would
        return lut

    def assign_consensus_labels(self, external_data: pd.DataFrame) -> pd.DataFrame:
        """``external_data`` with the meta cluster of every row's SOM cluster in ``meta_col``."""
        external_data[self.meta_col] = external_data[self.som_col].map(
            self.mapping.set_index(self.som_col)[self.meta_col])
        return external_data
