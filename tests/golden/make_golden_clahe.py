"""Writes g30_clahe.npz: per case of tests/clahe_reference.fixture_cases() the K27 statement's equalize_adapthist(plane, k,
clip_limit) -- the float64 result in full and, for the cases of at most FULL_LIMIT pixels, `gray`, `maps` and `raw` in full
(uint16); for the larger ones the SHA-256 of their bytes, so equality stays checkable bit for bit within g29's order of
size.  Everything comes from numpy and scipy; the inputs are clahe_reference's seeded patterns after the sigma = 2 blur and
the division by the maximum, so only results are stored.

The cases: noisy bars of period 6 at 64 x 64 with k = 32 under the default clip limit (clim = 10), under clip_limit = 0.003
on a smooth pattern (clim = 3, 768 < 1024 pixels: the loop walks all 256 indices twice and ends without progress) and
without clipping; k = 8 (clim = 1) and k = 16 (clim = 2) on 16 x 16 .. 40 x 24, the reference's own regime, where the first
phase does nothing and the loop does the work; a constant plane; a single bright pixel; odd k (3, 5, 7) on sizes that are no
multiple of k; k = 1 on 6 x 6; 128 x 128 with k = 8, the reference's 1024 / 128 in small.  One more case, `chain`, is a raw
channel carried through contrast_adjust (blur 2, k = 8) and then every K26 and K25 stage.

Counted here, per case: the tiles that reach each branch of clip_histogram (clahe_reference.BRANCHES).  Asserted: the file
as a whole reaches every one of them; every result lies in [0, 1] and attains both ends unless the plane is constant; the
chained case has all three marker classes.

PXSOM_GOLDEN_OUT: the folder to write to (default: this one)."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import clahe_reference as cr  # noqa: E402
from tests import fiber_markers_reference as fmr  # noqa: E402
from tests import frangi_reference as fr  # noqa: E402

CUTOFF, SOBEL_BLUR = 0.1, 1
CHAIN_BLUR, CHAIN_K = 2, 8


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    out_dir = os.environ.get("PXSOM_GOLDEN_OUT", HERE)
    data = {"cutoff": np.float64(CUTOFF), "sobel_blur": np.float64(SOBEL_BLUR), "chain_blur": np.float64(CHAIN_BLUR),
            "chain_k": np.int64(CHAIN_K), "branch_names": np.array(json.dumps(list(cr.BRANCHES)))}
    names, reached = [], dict.fromkeys(cr.BRANCHES, 0)
    for name, (x, k, clip_limit) in cr.fixture_cases().items():
        result, gray, maps, raw = cr.equalize_adapthist(x, k, clip_limit)
        assert result.dtype == np.float64 and gray.dtype == np.uint16 and raw.dtype == np.uint16 and gray.max() < cr.NR, name
        assert 0 <= maps.min() and maps.max() < cr.NR and maps.shape == (-(-x.shape[0] // k), -(-x.shape[1] // k), 256), name
        assert result.min() >= 0.0 and result.max() <= 1.0, name
        if x.min() != x.max():
            assert result.min() == 0.0 and result.max() == 1.0, name
        branches = cr.tile_branches(gray, k, clip_limit)
        for b, n in branches.items():
            reached[b] += n
        data["k_" + name], data["clip_limit_" + name] = np.int64(k), np.float64(clip_limit)
        data["clim_" + name] = np.int64(cr.clip_limit_count(k, clip_limit))
        data["branches_" + name] = np.array([branches[b] for b in cr.BRANCHES], np.int64)
        data["result_" + name] = result
        if x.size <= cr.FULL_LIMIT:
            data["gray_" + name], data["maps_" + name], data["raw_" + name] = gray, maps.astype(np.uint16), raw
        else:
            for key, a in (("gray", gray), ("maps", maps.astype(np.uint16)), ("raw", raw)):
                data["sha256_%s_%s" % (key, name)] = np.array(digest(a))
        names.append(name)
        print("%-18s %3d x %3d  k %2d  clim %5d  tiles %3d  %s" % (name, x.shape[0], x.shape[1], k, data["clim_" + name],
                                                                  maps.shape[0] * maps.shape[1],
                                                                  " ".join("%s=%d" % (b, n) for b, n in branches.items() if n)))
    missing = [b for b, n in reached.items() if n == 0]
    assert not missing, missing
    data["names"] = np.array(json.dumps(names))

    # the chained case: a raw channel through the whole front and every later stage
    channel = cr.chain_channel()
    contrast, gray, maps, raw = cr.contrast_adjust(channel, CHAIN_BLUR, CHAIN_K)
    ridges = fr.frangi(contrast, fr.SIGMAS, fr.BETA, fr.GAMMA, fr.SCALE)
    k25 = fmr.stages(ridges, CUTOFF, SOBEL_BLUR)
    classes = np.bincount(k25["markers"].ravel(), minlength=3)
    assert classes.shape == (3,) and classes.min() > 0, classes
    near = np.abs(k25["elev"] - np.rint(k25["elev"]))
    assert not ((near < 1e-9) & (np.rint(k25["elev"]) != 0)).any()
    data.update(chain_contrast=contrast, chain_gray=gray, chain_maps=maps.astype(np.uint16), chain_raw=raw, chain_ridges=ridges,
                chain_thr=np.array([k25["t0"], k25["t1"]]))
    for key in ("fg", "dist", "counts", "markers", "elev", "elevation"):
        data["chain_" + key] = k25[key]
    print("chain              %3d x %3d  marker classes %s" % (channel.shape[0], channel.shape[1], classes.tolist()))
    np.savez_compressed(os.path.join(out_dir, "g30_clahe.npz"), **data)
    print("reached: " + " ".join("%s=%d" % (b, n) for b, n in reached.items()))


if __name__ == "__main__":
    main()
