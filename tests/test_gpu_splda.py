"""pxsom_neighborhood_sums on the GPU against the numpy statement of tests/splda_reference.py, bit for bit (no tolerance),
and the spatial-LDA preprocessing on the HIP path through the checks of tests/test_splda.py."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import splda_reference as sr
from tests import test_splda as ts

pytestmark = pytest.mark.gpu

FOV_SIZES = [0, 1, 0, 2, 0, 255, 0, 256, 0, 257, 0, 600]      # the candidate tile edge at 256, an empty FOV between
FEATURE_COUNTS = [0, 1, 7, 8, 9, 17, 64]                       # the feature chunk edges at 8
RADII = [25, 32, 50, 64]                                       # two of them powers of two
MAX_FEAT = max(FEATURE_COUNTS)
# integer offsets exactly `radius` long: the axes for every radius, and the Pythagorean ones 25 and 50 have
AT_RADIUS = {25: [(25, 0), (0, 25), (15, 20), (7, 24)], 32: [(32, 0), (0, 32)],
             50: [(50, 0), (0, 50), (30, 40), (14, 48)], 64: [(64, 0), (0, 64)]}

_COHORTS, _STATEMENTS = {}, {}


def cohort(radius):
    """FOVs of FOV_SIZES on square fields sized for about 10 neighbours within ``radius``, with 64 feature columns.  The
    last FOV (600 cells) also holds: cells on another cell's centroid; an anchor at integer coordinates with one cell at
    every offset of AT_RADIUS[radius]; a cell with a NaN and, elsewhere, one with a +inf in feature column 0; a cell
    with NaN coordinates.  Returns a dict, built once per radius and never changed."""
    if radius in _COHORTS:
        return _COHORTS[radius]
    rs = np.random.RandomState(radius)
    xy = []
    for m in FOV_SIZES:
        side = max(np.sqrt(m * np.pi * radius ** 2 / 10.0), 1.0)
        xy.append(rs.uniform(0, side, (m, 2)))
    big = xy[-1]
    big[10:16] = big[20:26]                                    # on another cell's centroid
    anchor = 100
    big[anchor] = (120.0, 130.0)
    partners = []
    for j, (dx, dy) in enumerate(AT_RADIUS[radius]):
        big[anchor + 1 + j] = (120.0 + dx, 130.0 + dy)
        partners.append(anchor + 1 + j)
    nan_xy = 300
    big[nan_xy] = (np.nan, 40.0)
    seg = np.concatenate([[0], np.cumsum(FOV_SIZES)]).astype(np.int64)
    xy = np.ascontiguousarray(np.concatenate(xy))
    feats = rs.uniform(-1, 1, (len(xy), MAX_FEAT))
    feats[rs.uniform(size=feats.shape) < 0.05] = 0.0
    off = int(seg[-2])
    nan_cell, inf_cell = off + 400, off + 500
    feats[nan_cell, 0] = np.nan
    feats[inf_cell, 0] = np.inf
    c = dict(xy=xy, feats=feats, seg=seg, anchor=off + anchor, partners=[off + p for p in partners],
             nan_xy=off + nan_xy, nan_cell=nan_cell, inf_cell=inf_cell, last=(off, int(seg[-1])))
    for a in (xy, feats, seg):
        a.setflags(write=False)
    _COHORTS[radius] = c
    return c


def statement(radius, closed):
    """The statement's (sums over all 64 columns, counts), once per (radius, closed): the sums of the first p columns
    are its first p columns, since every column is folded on its own."""
    key = (radius, closed)
    if key not in _STATEMENTS:
        c = cohort(radius)
        _STATEMENTS[key] = sr.neighborhood_sums(c["xy"], c["feats"], c["seg"], radius, closed)
    return _STATEMENTS[key]


def _device(gpu, xy, feats, seg, radius, closed):
    from ark_analysis_amd import som_device
    sums, counts = som_device.neighborhood_sums(
        torch.from_numpy(np.array(xy)).to(gpu), None if feats is None else torch.from_numpy(np.array(feats)).to(gpu),
        torch.from_numpy(np.array(seg)).to(gpu), radius, closed)
    torch.cuda.synchronize()
    assert sums.dtype == torch.float64 and counts.dtype == torch.int32
    assert tuple(sums.shape) == (len(xy), 0 if feats is None else feats.shape[1]) and tuple(counts.shape) == (len(xy),)
    return sums.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("n_feat", FEATURE_COUNTS)
def test_kernel_equals_statement(gpu, n_feat, radius):
    c = cohort(radius)
    feats = None if n_feat == 0 else np.ascontiguousarray(c["feats"][:, :n_feat])
    got = {}
    for closed in (False, True):
        sums, counts = got[closed] = _device(gpu, c["xy"], feats, c["seg"], radius, closed)
        want_sums, want_counts = statement(radius, closed)
        bad = np.flatnonzero(counts != want_counts)
        assert bad.size == 0, (closed, bad[:5], counts[bad[:5]], want_counts[bad[:5]])
        assert np.array_equal(sums, want_sums[:, :n_feat], equal_nan=True), closed
    # the cells exactly at the radius: out under "lt", in under "le"
    lt, le = got[False][1], got[True][1]
    assert le[c["anchor"]] - lt[c["anchor"]] == len(c["partners"])
    for p in c["partners"]:
        assert le[p] - lt[p] >= 1
    assert lt[c["nan_xy"]] == 0 and le[c["nan_xy"]] == 0
    if n_feat:
        # the NaN and the +inf reach exactly the rows within the radius of their cells
        a, b = c["last"]
        for closed in (False, True):
            col = got[closed][0][:, 0]
            near_nan = np.zeros(len(col), bool)
            near_inf = np.zeros(len(col), bool)
            near_nan[a:b] = sr._mask(c["xy"][a:b], c["nan_cell"] - a, np.float64(radius), closed)
            near_inf[a:b] = sr._mask(c["xy"][a:b], c["inf_cell"] - a, np.float64(radius), closed)
            assert near_nan.sum() >= 1 and near_inf.sum() >= 1
            assert np.array_equal(np.isnan(col), near_nan)
            assert np.array_equal(np.isposinf(col), near_inf & ~near_nan)
            assert np.isfinite(got[closed][0][:, 1:]).all()


@pytest.mark.parametrize("n_feat", [0, 9])
def test_workgroups_that_span_many_fovs(gpu, n_feat):
    """100 FOVs of 3 cells: two workgroups, each visiting dozens of FOVs."""
    rs = np.random.RandomState(100 + n_feat)
    xy = rs.uniform(0, 60, (300, 2))
    feats = rs.uniform(-1, 1, (300, n_feat)) if n_feat else None
    seg = np.arange(0, 301, 3, dtype=np.int64)
    for closed in (False, True):
        sums, counts = _device(gpu, xy, feats, seg, 32, closed)
        want_sums, want_counts = sr.neighborhood_sums(xy, feats, seg, 32, closed)
        assert np.array_equal(counts, want_counts) and 1 <= counts.min() and counts.max() <= 3 and (counts < 3).any()
        assert np.array_equal(sums, want_sums, equal_nan=True)


def test_no_cells_and_argument_errors(gpu):
    from ark_analysis_amd import som_device
    for seg in ([0], [0, 0, 0]):
        sums, counts = _device(gpu, np.zeros((0, 2)), np.zeros((0, 3)), np.array(seg, dtype=np.int64), 50, False)
        assert sums.shape == (0, 3) and counts.shape == (0,)
    xy = torch.zeros((4, 2), dtype=torch.float64, device=gpu)
    seg = torch.tensor([0, 4], device=gpu)
    with pytest.raises(ValueError, match="feats must be"):
        som_device.neighborhood_sums(xy, torch.zeros((3, 2), dtype=torch.float64, device=gpu), seg, 50)
    with pytest.raises(ValueError, match="feats must be"):
        som_device.neighborhood_sums(xy, torch.zeros((4, 2), dtype=torch.float32, device=gpu), seg, 50)
    with pytest.raises(ValueError, match="seg must be non-decreasing"):
        som_device.neighborhood_sums(xy, None, torch.tensor([0, 3], device=gpu), 50)
    with pytest.raises(ValueError, match="xy must be"):
        som_device.neighborhood_sums(xy.cpu(), None, seg, 50)
    # a NaN radius is below nothing
    sums, counts = som_device.neighborhood_sums(xy, torch.ones((4, 2), dtype=torch.float64, device=gpu), seg, float("nan"))
    assert counts.cpu().tolist() == [0] * 4 and sums.cpu().abs().sum().item() == 0.0


# ---- the public layer on the HIP path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("featurization", ts.FEATURIZATIONS)
def test_featurization_equals_the_pandas_loop(gpu, featurization):
    from ark_analysis_amd.spLDA import processing as pros
    ts.check_featurization(pros, featurization)


def test_featurize_cell_table_dict_and_split(gpu):
    from ark_analysis_amd.spLDA import processing as pros
    ts.check_featurize_cell_table(pros)


def test_radius_test_le_takes_the_cells_at_the_radius(gpu, monkeypatch):
    from ark_analysis_amd.spLDA import processing as pros
    df = pd.DataFrame({"x": [0.0, 30.0, 50.0, 0.0], "y": [0.0, 40.0, 0.0, 50.0], "cluster": ["a"] * 4,
                       "is_index": [True] * 4})
    table = {"f": df, "fovs": np.array(["f"]), "markers": None, "clusters": ["a"]}
    assert pros.neighborhood_features(table, "count", 50)["count"].tolist()[0] == 1
    monkeypatch.setattr(pros, "RADIUS_TEST", "le")
    assert pros.neighborhood_features(table, "count", 50)["count"].tolist()[0] == 4


def test_within_cluster_sums_device_route(gpu):
    from ark_analysis_amd.utils import spatial_lda_utils as spu
    ts.check_within_cluster_sums_device(spu)


def test_silhouette_sums_are_what_the_samples_are_made_of(gpu):
    """silhouette_sums returns pxsom_silhouette's own sums and counts; the present callers' results are untouched."""
    from ark_analysis_amd import som_device
    rs = np.random.RandomState(6)
    x = torch.from_numpy(rs.normal(size=(200, 5))).to(gpu)
    labels = torch.from_numpy(rs.randint(0, 4, 200)).to(gpu)
    sums, counts = som_device.silhouette_sums(x, labels, 4)
    assert tuple(sums.shape) == (1, 200, 4) and tuple(counts.shape) == (1, 4)
    assert counts[0].cpu().tolist() == np.bincount(labels.cpu().numpy(), minlength=4).tolist()
    want, _ = sr.silhouette_sums_stand_in(x.cpu().numpy(), labels.cpu().numpy(), 4)
    np.testing.assert_allclose(sums[0].cpu().numpy(), want, rtol=(5 + 2 + 200) * 2 * ts.U, atol=0)
    samples, scores, single = som_device._silhouette(x, labels, 4)
    assert single and torch.equal(samples[0], som_device.silhouette_samples(x, labels, 4))
    assert torch.equal(scores, som_device.silhouette_scores(x, labels, 4))


def test_topic_eda_device(gpu):
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    from ark_analysis_amd.spLDA import processing as pros
    ts.check_topic_eda_device(pros, sau)
