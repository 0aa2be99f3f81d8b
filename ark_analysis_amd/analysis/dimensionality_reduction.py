"""Mirror of the reference's ``ark.analysis.dimensionality_reduction``: the 2-D projection of the cell table's marker
columns and its scatter plot, with PCA and exact t-SNE on the device (K30, DESIGN.md "K30").

Deliberate deviations from ``sklearn.manifold.TSNE()`` as the reference calls it:

* the gradient is exact, where sklearn's default is Barnes-Hut at angle 0.5;
* the embedding is binary64 throughout, where sklearn keeps it in float32;
* the PCA initialisation comes from the exact covariance route, where sklearn uses the randomized solver.

The optimiser is otherwise sklearn 1.7.2's ``TSNE._tsne`` and ``_gradient_descent`` (learning rate ``max(n / 48, 50)``,
early exaggeration 12 for 250 iterations at momentum 0.5, then momentum 0.8).  The reference itself gives different
coordinates on every call (``random_state=None``), so parity is by objective and structure, not by coordinates.
"""
import os

import numpy as np

from ..host_utils import verify_in_list

ALGORITHMS = ["UMAP", "PCA", "tSNE"]
_FILES = {"UMAP": "UMAPVisualization.png", "PCA": "PCAVisualization.png", "tSNE": "tSNEVisualization.png"}
_FIG_IDS = {"UMAP": 1, "PCA": 2, "tSNE": 3}


class EmbeddingResult(np.ndarray):
    """The ``[n, 2]`` embedding; after t-SNE it carries ``kl_divergence_`` and ``n_iter_`` as sklearn's estimator does."""
    kl_divergence_ = None
    n_iter_ = None


def _embed_device(values, algorithm, random_state, perplexity, max_iter, init):
    """The device route: the host table in, ``(embedding [n, 2] float64, kl_divergence or None, n_iter or None)`` out."""
    import torch

    from .. import _capi, som_device
    dev = _capi.require_gpu()
    x = torch.from_numpy(values).to(dev)
    if algorithm == "PCA":
        return som_device.pca_scores(x).cpu().numpy(), None, None
    res = som_device.tsne_embed(x, perplexity=perplexity, max_iter=max_iter, init=init, random_state=random_state)
    return res.embedding.cpu().numpy(), res.kl_divergence, res.n_iter


def _embed_umap(values):
    try:
        import umap
    except ImportError as e:
        raise ImportError('algorithm "UMAP" needs the umap-learn package, which does not import here; '
                          '"tSNE" and "PCA" run on the device without it') from e
    from sklearn.preprocessing import StandardScaler
    return umap.UMAP().fit_transform(StandardScaler().fit_transform(values))


def reduce_dimensions(values, algorithm, *, random_state=None, perplexity=30.0, max_iter=1000, init="pca"):
    """Two components of ``values`` (``[n, c]``, float32 stays float32 on the device, anything else goes as float64).

    ``"PCA"``: sklearn's ``PCA().fit_transform(values)[:, :2]`` -- column means, the centred covariance over n - 1, its
    eigenvectors, each signed so that its loading of largest magnitude is positive.  ``"tSNE"``: exact t-SNE with Euclidean
    input distances (see the module docstring for what differs from ``TSNE()``); ``init`` is ``"pca"``, ``"random"`` or an
    ``[n, 2]`` array, and the result carries ``kl_divergence_`` and ``n_iter_``.  ``"UMAP"``: the reference's host code when
    ``umap`` imports, else ImportError.  There is no host fallback for PCA and t-SNE: a table too large for the device
    raises NotImplementedError naming the largest that fits."""
    verify_in_list(algorithm=algorithm, dimensionality_reduction_algorithms=ALGORITHMS)
    values = np.asarray(values)
    if values.ndim != 2:
        raise ValueError("values must be a 2-D [rows, columns] table, got shape %s" % (values.shape,))
    values = np.ascontiguousarray(values, dtype=np.float32 if values.dtype == np.float32 else np.float64)
    if not np.isfinite(values).all():
        raise ValueError("Input X contains NaN or infinity.")
    n, c = values.shape
    if algorithm == "UMAP":
        return np.asarray(_embed_umap(values)).view(EmbeddingResult)
    if algorithm == "PCA":
        if n < 2 or c < 2:
            raise ValueError("PCA needs at least 2 rows and 2 columns, got %d x %d" % (n, c))
    else:
        if c < 1:
            raise ValueError("tSNE needs at least 1 column")
        if perplexity >= n:
            raise ValueError("perplexity must be less than n_samples")
        if not perplexity > 0:
            raise ValueError("perplexity must be positive, got %r" % (perplexity,))
        if max_iter < 250:
            raise ValueError("max_iter must be at least 250, got %r" % (max_iter,))
        if isinstance(init, str):
            if init not in ("pca", "random"):
                raise ValueError("init must be 'pca', 'random' or an [n, 2] array, got %r" % (init,))
            if init == "pca" and c < 2:
                raise ValueError("init='pca' needs at least 2 columns")
        else:
            init = np.ascontiguousarray(init, dtype=np.float64)
            if init.shape != (n, 2) or not np.isfinite(init).all():
                raise ValueError("init must be a finite array of shape (%d, 2)" % n)
    emb, kl, n_iter = _embed_device(values, algorithm, random_state, perplexity, max_iter, init)
    out = np.ascontiguousarray(emb, dtype=np.float64).view(EmbeddingResult)
    out.kl_divergence_, out.n_iter_ = kl, n_iter
    return out


def plot_dim_reduced_data(component_one, component_two, fig_id, hue, cell_data, title, title_fontsize=24,
                          palette="Spectral", alpha=0.3, legend_type="full", bbox_to_anchor=(1.05, 1), legend_loc=2,
                          legend_borderaxespad=0., dpi=None, save_dir=None, save_file=None):
    """The reference's helper with matplotlib alone: one scatter per category of ``hue`` (sorted), coloured at equal steps
    of the colormap ``palette``, then the legend, the title and, with ``save_dir``, the file.  The reference draws with
    seaborn's ``scatterplot``; pixel parity with it is unpinned (marker size, edge colour and the exact palette sampling
    are seaborn's).  ``legend_type=False`` leaves the legend entries out; ``cell_data`` is accepted for the signature."""
    import matplotlib
    import matplotlib.pyplot as plt

    x, y, hue = np.asarray(component_one), np.asarray(component_two), np.asarray(hue)
    plt.figure(fig_id)
    cats = sorted(set(hue.tolist()), key=lambda v: (str(type(v)), v))
    cmap = matplotlib.colormaps[palette]
    for k, cat in enumerate(cats):
        pick = hue == cat
        colour = cmap((k + 0.5) / len(cats))
        plt.scatter(x[pick], y[pick], color=colour, alpha=alpha, label=str(cat) if legend_type else None)
    if legend_type:
        plt.legend(bbox_to_anchor=bbox_to_anchor, loc=legend_loc, borderaxespad=legend_borderaxespad)
    plt.title(title, fontsize=title_fontsize)
    if save_dir is not None:
        if not os.path.isdir(save_dir):
            raise FileNotFoundError("save_dir %s does not exist" % save_dir)
        plt.savefig(os.path.join(save_dir, save_file), dpi=dpi)


def visualize_dimensionality_reduction(cell_data, columns, category, color_map="Spectral", algorithm="UMAP", dpi=None,
                                       save_dir=None, *, random_state=None, perplexity=30.0, max_iter=1000):
    """Plots the dimensionality reduction of the population ``columns`` of ``cell_data``, coloured by ``category``: the
    reference's function, with ``"PCA"`` and ``"tSNE"`` on the device (``reduce_dimensions``).  Rows with a NaN anywhere
    are dropped first, as the reference does.  Returns the ``[n, 2]`` embedding (the reference returns None)."""
    cell_data = cell_data.dropna()
    verify_in_list(algorithm=algorithm, dimensionality_reduction_algorithms=ALGORITHMS)
    graph_title = "%s projection of data" % algorithm
    embedding = reduce_dimensions(cell_data[columns].values, algorithm, random_state=random_state, perplexity=perplexity,
                                  max_iter=max_iter)
    plot_dim_reduced_data(embedding[:, 0], embedding[:, 1], fig_id=_FIG_IDS[algorithm], hue=cell_data[category],
                          cell_data=cell_data, title=graph_title, dpi=dpi, save_dir=save_dir, save_file=_FILES[algorithm],
                          palette=color_map)
    return embedding
