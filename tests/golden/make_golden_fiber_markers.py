"""Writes g28_fiber_markers.npz: small foreground planes and, per plane, every stage of K25 as scipy and numpy compute it
(tests/fiber_markers_reference.py): the squared distances (brute force), the smoothed distance map, the 256 counts, the
thresholds under every RECALLED_MULTIOTSU setting of `prob` and `tie`, the markers, the Sobel magnitude and its int32
form.  The ridge plane of a case is fiber_markers_reference.ridge_plane(fg), so only fg is stored.

The conditions the tests rely on are asserted here, on the inputs:
  * all three marker classes are non-empty;
  * the thresholds are the same under float32 and binary64 `prob`;
  * no pixel of the Sobel magnitude lies within 1e-9 of a non-zero integer (its int32 form does not hang on a rounding);
  * scipy.ndimage.sobel equals the two correlate1d stages bit for bit;
  * scipy's distance transform equals the square root of the brute-force squared distance bit for bit.

PXSOM_GOLDEN_OUT: the folder to write to (default: this one)."""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from ark_analysis_amd.segmentation import fiber_segmentation as fs  # noqa: E402
from tests import fiber_markers_reference as fmr  # noqa: E402

CUTOFF, SOBEL_BLUR = 0.1, 1
SETTINGS = [dict(prob=p, tie=t) for p, t in itertools.product(fs.MULTIOTSU_CHOICES["prob"], fs.MULTIOTSU_CHOICES["tie"])]


def planes():
    seeds = iter(range(28, 40))                      # one stream per plane: changing a plane leaves the others alone

    def rs_next():
        return np.random.RandomState(next(seeds))

    out = {}
    out["bars"] = fmr.bars(64, 64, rs_next(), 6)
    out["bars_small"] = fmr.bars(40, 40, rs_next(), 4)
    rs = rs_next()
    speckle = fmr.bars(40, 40, rs, 4)
    speckle[rs.random_sample(speckle.shape) < 0.02] ^= 1
    out["speckle"] = speckle
    yy, xx = np.mgrid[:40, :40]
    out["disc"] = ((yy - 19) ** 2 + (xx - 21) ** 2 <= 11 ** 2).astype(np.uint8)
    blob = ((yy - 20) ** 2 / 1.6 + (xx - 18) ** 2 <= 14 ** 2).astype(np.uint8)
    blob[(yy - 22) ** 2 + (xx - 16) ** 2 <= 3 ** 2] = 0
    out["blob_hole"] = blob
    borders = fmr.bars(40, 40, rs_next(), 2)
    borders[:3] = borders[-2:] = 1
    borders[:, :2] = borders[:, -4:] = 1
    out["borders"] = borders
    out["wide"] = fmr.bars(40, 90, rs_next(), 5)
    out["tall"] = fmr.bars(90, 40, rs_next(), 5)
    return out


def main():
    out_dir = os.environ.get("PXSOM_GOLDEN_OUT", HERE)
    data = {"settings": np.array(json.dumps(SETTINGS)), "cutoff": np.float64(CUTOFF), "sobel_blur": np.float64(SOBEL_BLUR)}
    names = []
    for name, fg in planes().items():
        assert fg.dtype == np.uint8 and max(fg.shape) <= 96 and not fg.all() and fg.any(), name
        s = fmr.stages(fmr.ridge_plane(fg, CUTOFF), CUTOFF, SOBEL_BLUR)
        assert np.array_equal(s["fg"], fg), name
        sq = fmr.squared_distances(fg)
        assert np.array_equal(np.sqrt(sq.astype(np.float64)), fmr.distance_transform_edt(fg)), name
        thr = np.array([fs.threshold_multiotsu_from_histogram(s["counts"], s["edges"], recalled=r) for r in SETTINGS])
        by_prob = {p: thr[[i for i, r in enumerate(SETTINGS) if r["prob"] == p]] for p in fs.MULTIOTSU_CHOICES["prob"]}
        assert np.array_equal(by_prob["float32"], by_prob["float64"]), (name, thr)
        assert np.array_equal(thr[0], [s["t0"], s["t1"]]), name
        classes = np.bincount(s["markers"].ravel(), minlength=3)
        assert classes.shape == (3,) and classes.min() > 0, (name, classes)
        near = np.abs(s["elev"] - np.rint(s["elev"]))
        assert not ((near < 1e-9) & (np.rint(s["elev"]) != 0)).any(), name
        smooth = fmr.blur(s["dist"], SOBEL_BLUR)
        for got, want in zip(fmr.sobel_separable(smooth), fmr.sobel_axes(smooth)):
            assert np.array_equal(got, want), name
        for key, value in (("fg", fg), ("sq", sq), ("dist", s["dist"]), ("counts", s["counts"]), ("thr", thr),
                           ("markers", s["markers"]), ("elev", s["elev"]), ("elevation", s["elevation"])):
            data["%s_%s" % (key, name)] = value
        names.append(name)
        print("%-11s %3d x %3d  fg %5.1f %%  classes %s  thresholds %s  elevation max %d" % (
            name, fg.shape[0], fg.shape[1], 100.0 * fg.mean(), classes.tolist(), np.round(thr[0], 4).tolist(), s["elevation"].max()))
    data["names"] = np.array(json.dumps(names))
    np.savez_compressed(os.path.join(out_dir, "g28_fiber_markers.npz"), **data)


if __name__ == "__main__":
    main()
