#!/usr/bin/env python
"""Generates tests/golden/g25_projection_masks.npz: "projection" object masks of the REFERENCE's
ark.segmentation.ez_seg.ez_object_segmentation._create_object_mask, imported as make_golden_object_masks.py imports it
(same shims, same restated skimage functions), plus the bare ridge masks of the fixture images.

The seventh skimage function the reference calls on this branch, filters.meijering, is restated here from skimage 0.19's
algorithm as recalled (scikit-image is not a dependency here, and the reference pins scikit-image < 0.19.3):
  - the image as float: x = (image != 0) in binary64 (img_as_float of a boolean plane; the 0 / 1 integer plane that
    hole_size=None hands over is taken the same way)
  - per sigma: hessian_matrix(x, sigma, mode="reflect", order="rc") = np.gradient twice on
    scipy.ndimage.gaussian_filter(x, sigma, mode="reflect"), each element times sigma ** 2
  - np.linalg.eigvalsh of the symmetric 2 x 2 matrices, sorted by magnitude (a tie keeps eigvalsh's smaller value first)
  - the value of larger magnitude plus alpha = 1 / ndim times the other; what is not negative becomes 0
  - _divide_nonzero by the plane's minimum, then the maximum over the sigmas
Parity with skimage itself is therefore UNPINNED, as for the six functions of make_golden_object_masks.py; skimage >= 0.20
rewrote the ridge filters and is not what is stated here.  The reference only uses `> 0` of the result.

Per image the generator asserts that the closed-form statement of tests/projection_mask_reference.py (no eigvalsh, no
normalisation) gives the same mask on every pixel.  The fixtures hold inputs, parameters and expected masks -- no
reference text.

    python tests/golden/make_golden_projection_masks.py      (needs /root/reference; never runs on the GPU box)
    PXSOM_GOLDEN_OUT=<dir> ... writes to <dir> instead, to compare a regeneration with the committed file.
"""
import json
import sys

import numpy as np
import scipy.ndimage as ndi

import make_golden_object_masks as base

from tests import projection_mask_reference as pmr  # noqa: E402  (base put the repository root on sys.path)


# ---- the restated filter ------------------------------------------------------------------------------------------------
def _divide_nonzero(array1, array2, cval=1e-10):
    denominator = np.copy(array2)
    denominator[denominator == 0] = cval
    return np.divide(array1, denominator)


def meijering(image, sigmas=range(1, 10, 2), alpha=None, black_ridges=True, mode="reflect", cval=0):
    assert not black_ridges and mode == "reflect"
    x = (np.asarray(image) != 0).astype(np.float64)
    alpha = 1.0 / x.ndim if alpha is None else alpha
    filtered = np.zeros((len(list(sigmas)),) + x.shape)
    for i, sigma in enumerate(sigmas):
        g = ndi.gaussian_filter(x, sigma, mode=mode, cval=cval)
        grads = np.gradient(g)
        s2 = float(sigma ** 2)
        hrr, hrc, hcc = s2 * np.gradient(grads[0], axis=0), s2 * np.gradient(grads[0], axis=1), s2 * np.gradient(grads[1], axis=1)
        matrices = np.stack([np.stack([hrr, hrc], axis=-1), np.stack([hrc, hcc], axis=-1)], axis=-2)
        ev = np.linalg.eigvalsh(matrices)                                   # ascending along the last axis
        order = np.argsort(-np.abs(ev), axis=-1, kind="stable")             # larger magnitude first, a tie keeps the order
        ev = np.take_along_axis(ev, order, axis=-1)
        aux = ev[..., 0] + alpha * ev[..., 1]
        aux = np.where(aux < 0, aux, 0)
        filtered[i] = _divide_nonzero(aux, np.full_like(aux, aux.min()))
    return filtered.max(axis=0)


# ---- inputs -------------------------------------------------------------------------------------------------------------
def images():
    """Eight intensity images (float32) whose `> 0` plane is the pattern named: the values vary so that a percentile
    threshold has something to cut."""
    rs = np.random.RandomState(251)
    shapes = {"lines": pmr.lines(96, 80, rs), "discs": pmr.discs(72, 96, rs), "ring": pmr.ring(64, 70),
              "noise": pmr.noise(50, 66, rs), "quadrant": pmr.quadrant(64, 64, 32, 32), "mixed": pmr.lines(90, 96, rs) | pmr.discs(90, 96, rs),
              "tiny": pmr.noise(3, 5, rs, 0.5), "flat": pmr.lines(2, 9, rs, 2)}
    return {k: (m * rs.randint(3, 60, m.shape)).astype(np.float32) for k, m in shapes.items()}


CASES = [  # (name, image, sigma, thresh, hole_size, fov_dim, min_object_area, max_object_area)
    ("lines_none_none", "lines", 1, None, None, 100, 10, 100000),
    ("lines_pct_int", "lines", 1, 30, 12, 100, 5, 100000),
    ("lines_auto_auto", "lines", 1, "auto", "auto", 100, 5, 100000),
    ("discs_none_int", "discs", 1, None, 20, 100, 10, 100000),
    ("discs_pct_auto", "discs", 2, 40, "auto", 100, 10, 100000),
    ("discs_auto_none", "discs", 1, "auto", None, 100, 4, 100000),
    ("ring_none_auto", "ring", 1, None, "auto", 100, 10, 100000),
    ("ring_pct_none", "ring", None, 20, None, 100, 1, 100000),
    ("noise_auto_int", "noise", 1, "auto", 6, 100, 3, 100000),
    ("noise_none_none", "noise", None, None, None, 100, 2, 50),
    ("quadrant_none_none", "quadrant", None, None, None, 100, 1, 100000),
    ("quadrant_pct_int", "quadrant", 1, 50, 5, 100, 1, 100000),
    ("mixed_none_int", "mixed", 1, None, 15, 100, 10, 100000),
    ("mixed_auto_auto", "mixed", 2, "auto", "auto", 200, 8, 4000),
    ("tiny_none_none", "tiny", None, None, None, 100, 1, 100000),
    ("tiny_none_int", "tiny", 1, None, 2, 100, 1, 100000),
    ("flat_none_none", "flat", None, None, None, 100, 1, 100000),
    ("flat_pct_int", "flat", 1, 10, 3, 100, 1, 100000),
]


def g25_projection_masks(ez):
    imgs = images()
    out = {"img_" + k: v for k, v in imgs.items()}
    for key, img in imgs.items():
        plane = img > 0
        by_eigvalsh = meijering(plane, sigmas=range(1, 5, 1), black_ridges=False) > 0
        closed = pmr.ridge_sign(plane) != 0
        assert np.array_equal(by_eigvalsh, closed), (key, int((by_eigvalsh != closed).sum()))
        out["ridge_" + key] = by_eigvalsh.astype(np.uint8)
    meta = []
    for name, key, sigma, thresh, hole, fov_dim, lo, hi in CASES:
        mask = ez._create_object_mask(imgs[key].copy(), "projection", sigma, thresh, hole, fov_dim, lo, hi)
        assert mask.dtype == np.int32
        out["mask_" + name] = mask
        meta.append(dict(name=name, image=key, sigma=sigma, thresh=thresh, hole_size=hole, fov_dim=fov_dim,
                         min_object_area=lo, max_object_area=hi))
    out["cases"] = np.array(json.dumps(meta))
    base.save("g25_projection_masks", **out)


if __name__ == "__main__":
    ez, _ = base.inject()
    sys.modules["skimage.filters"].meijering = meijering
    g25_projection_masks(ez)
