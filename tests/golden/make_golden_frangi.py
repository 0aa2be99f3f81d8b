"""Writes g29_frangi.npz: small float64 planes and, per plane, the K26 statement of tests/frangi_reference.py at the
reference's widths (1, 3, 5, 7, 9): the per-scale vesselness (`scales`), their maximum (`folded`) and `ridges` = folded *
10000.  Everything comes from numpy and scipy; the inputs are frangi_reference's seeded patterns, so only results are stored.

The planes: noisy bright bars, the same bars dark on bright, a disc, a constant plane (every eigenvalue 0: the 1e-10
denominator), a linear ramp, a single bright pixel, K22's quadrant (|lambda| ties), the bars times 1e6 (rg / gsq beyond
708: exp_neg returns 0), and bars at 40 x 90 and 90 x 40.  Two cases (CHAINED) also carry every K25 stage computed from
their `ridges` by tests/fiber_markers_reference.py.

Size: the file stays below g28's 207 KB.  Stored in full, the per-scale planes of the two 3600-pixel cases alone would
take that, so the pattern cases are 16 to 28 pixels a side (the border rules reach two pixels), and the two large cases
store `ridges` in full and the SHA-256 of the bytes of `scales` and `folded`: equality stays checkable bit for bit.

Asserted here, on the statement:
  * E, the largest relative gap of exp_neg to np.exp over frangi_reference.exp_neg_grid(), in units of 2^-53, is recorded;
    with np.exp in exp_neg's place no per-scale plane of any case moves by more than (2 E + 2) * 2^-53 absolute: both
    factors lie in [0, 1], each carries E units, one rounding for the subtraction and one for the product;
  * the constant plane's Hessian is exactly zero and its result 0; the 1e6 case holds pixels whose second factor is exactly 1;
  * the quadrant holds a pixel where |e_lo| == |e_hi| at some scale;
  * the chained cases have all three marker classes.
The dark bars are NOT all zero: a dark bar's bright shoulders curve downwards across it and respond (only the bar's own
axis is silent), so that is recorded as the share of zero pixels, not asserted.

PXSOM_GOLDEN_OUT: the folder to write to (default: this one)."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import fiber_markers_reference as fmr  # noqa: E402
from tests import frangi_reference as fr  # noqa: E402

CUTOFF, SOBEL_BLUR = 0.1, 1
CHAINED = ("bars", "disc")
DIGESTED = ("wide", "tall")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    out_dir = os.environ.get("PXSOM_GOLDEN_OUT", HERE)
    gap_e = fr.exp_neg_gap(fr.exp_neg_grid())
    bound = (2.0 * gap_e + 2.0) * 2.0 ** -53
    data = {"sigmas": np.array(fr.SIGMAS, np.float64), "beta": np.float64(fr.BETA), "gamma": np.float64(fr.GAMMA),
            "scale": np.float64(fr.SCALE), "cutoff": np.float64(CUTOFF), "sobel_blur": np.float64(SOBEL_BLUR),
            "exp_gap_e": np.float64(gap_e)}
    names, observed = [], 0.0
    for name, x in fr.fixture_planes().items():
        assert x.dtype == np.float64 and min(x.shape) >= 2 and max(x.shape) <= 90, name
        s = fr.stages(x)
        other = fr.stages(x, exp=fr.np_exp)
        gap = float(np.abs(s["scales"] - other["scales"]).max())
        assert gap <= bound, (name, gap, bound)
        observed = max(observed, gap)
        assert not np.isnan(s["ridges"]).any() and np.array_equal(s["ridges"], s["folded"] * 10000.0), name
        assert np.array_equal(s["folded"], np.maximum.reduce(np.concatenate([np.zeros((1,) + x.shape), s["scales"]]))), name
        if name in DIGESTED:
            data["sha256_scales_" + name] = np.array(digest(s["scales"]))
            data["sha256_folded_" + name] = np.array(digest(s["folded"]))
        else:
            data["scales_" + name], data["folded_" + name] = s["scales"], s["folded"]
        data["ridges_" + name] = s["ridges"]
        if name in CHAINED:
            k25 = fmr.stages(s["ridges"], CUTOFF, SOBEL_BLUR)
            classes = np.bincount(k25["markers"].ravel(), minlength=3)
            assert classes.shape == (3,) and classes.min() > 0, (name, classes)
            near = np.abs(k25["elev"] - np.rint(k25["elev"]))
            assert not ((near < 1e-9) & (np.rint(k25["elev"]) != 0)).any(), name
            for key in ("fg", "dist", "counts", "markers", "elev", "elevation"):
                data["%s_%s" % (key, name)] = k25[key]
            data["thr_" + name] = np.array([k25["t0"], k25["t1"]])
        names.append(name)
        print("%-12s %3d x %3d  max %.6g  zero %5.1f %%  np.exp gap %.3g" % (
            name, x.shape[0], x.shape[1], s["folded"].max(), 100.0 * (s["folded"] == 0).mean(), gap))

    hessians = [fr.pmr.hessian(fr.fixture_planes()["constant"], sigma) for sigma in fr.SIGMAS]
    assert not any(np.any(h) for hs in hessians for h in hs) and not data["folded_constant"].any()
    gsq = 2.0 * fr.GAMMA ** 2
    hrr, hrc, hcc = fr.pmr.hessian(fr.fixture_planes()["bars_1e6"], 1)
    assert ((hrr * hrr + 2.0 * (hrc * hrc) + hcc * hcc) / gsq > 708.0).any()      # rg is the squared Frobenius norm
    tie = False
    for sigma in fr.SIGMAS:
        hrr, hrc, hcc = fr.pmr.hessian(fr.fixture_planes()["quadrant"], sigma)
        r = np.sqrt((hrr - hcc) ** 2 + 4.0 * (hrc * hrc))
        t = hrr + hcc
        tie |= bool(((np.abs((t - r) / 2.0) == np.abs((t + r) / 2.0)) & (r != 0)).any())
    assert tie
    data["names"] = np.array(json.dumps(names))
    data["exp_gap_observed"] = np.float64(observed * 2.0 ** 53)
    print("E = %.4f units of 2^-53 over %d arguments; largest np.exp gap of a vesselness plane %.4f units (bound %.4f)"
          % (gap_e, fr.exp_neg_grid().size, observed * 2.0 ** 53, 2.0 * gap_e + 2.0))
    np.savez_compressed(os.path.join(out_dir, "g29_frangi.npz"), **data)


if __name__ == "__main__":
    main()
