#!/usr/bin/env python
"""Generates tests/golden/g27_splda.npz: what the REFERENCE's ark.spLDA.processing and ark.utils.spatial_lda_utils give for
the functions that need none of spatial_lda's arithmetic -- format_cell_table (markers only, clusters only, both with a
cluster subset: the frames, their dtypes and the three bookkeeping keys), fov_density, within_cluster_sums on a 60 x 4
matrix with 3 labels, and the texts of the two argument checkers' errors -- imported from /root/reference/src with
tests/golden/_shims.

spatial_lda is not installed and cannot be: an empty-module stand-in (featurization, online_lda, visualization) goes
into sys.modules here, as do stand-ins for the plotting stack the reference's utility module imports and never calls on
these paths (seaborn, palettable, tqdm.notebook).  Nothing recorded here touches them.  What the recorded functions do
call is real: numpy, pandas, scipy's pdist, and the alpineer shim's verify_in_list.  The inputs and the list of calls
that must raise are in tests/splda_reference.py, which the test of the fixture shares.

    python tests/golden/make_golden_splda.py      (needs /root/reference; never runs on the GPU box)
    PXSOM_GOLDEN_OUT=<dir> ... writes to <dir> instead, to compare a regeneration with the committed file.
"""
import os
import sys
import types

import matplotlib

matplotlib.use("Agg")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "_shims"))
sys.path.insert(0, "/root/reference/src")

OUT_DIR = os.environ.get("PXSOM_GOLDEN_OUT", HERE)


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


# imported by the reference modules, never called by what is recorded here
_lda = _module("spatial_lda")
_lda.featurization = _module("spatial_lda.featurization")
_lda.online_lda = _module("spatial_lda.online_lda")
_lda.visualization = _module("spatial_lda.visualization", _standardize_topics=None, plot_adjacency_graph=None)
_module("seaborn")
_pal = _module("palettable")
_pal.colorbrewer = _module("palettable.colorbrewer")
_pal.colorbrewer.qualitative = _module("palettable.colorbrewer.qualitative",
                                       Set3_12=types.SimpleNamespace(mpl_colors=None))
_module("tqdm.notebook", tqdm=None)

from ark.spLDA import processing as ref_pr  # noqa: E402
from ark.utils import spatial_lda_utils as ref_spu  # noqa: E402

from tests import splda_reference as sr  # noqa: E402


def main():
    out = {}
    table = sr.golden_cell_table()
    sr.store_frame(out, "master_", table)
    formatted = {}
    for name, kwargs in sr.FORMAT_CASES.items():
        before = table.copy()
        formatted[name] = ref_pr.format_cell_table(table, **kwargs)
        assert table.equals(before)
        sr.record_formatted(out, "f_%s_" % name, formatted[name])
        dens = ref_pr.fov_density(formatted[name], total_pix=512 ** 2)
        for key in ("average_area", "cellular_density", "total_cells"):
            assert list(dens[key]) == list(formatted[name]["fovs"])
            out["d_%s_%s" % (name, key)] = np.asarray([dens[key][f] for f in formatted[name]["fovs"]])
    assert sorted(formatted["both"]["fovs"].tolist()) == ["fov12", "fov3", "fov8"]

    data, labels = sr.golden_within_case()
    out["w_data"], out["w_labels"] = data, labels
    out["w_sum"] = np.asarray(ref_spu.within_cluster_sums(data=data, labels=labels), dtype=np.float64)

    errors = sr.golden_errors(ref_spu, table, formatted["both"])
    assert "no error" not in errors.values(), errors
    out["e_names"] = np.array(list(errors))
    out["e_texts"] = np.array([errors[k] for k in errors])

    path = os.path.join(OUT_DIR, "g27_splda.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.relpath(path, ROOT), len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
