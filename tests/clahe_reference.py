"""The numpy / scipy statement of K27 (include/pxsom.h "K27"): the front of the reference's ``segment_fibers`` -- the sigma =
``blur`` Gaussian, the division by the maximum and skimage 0.19's ``equalize_adapthist(image, kernel_size,
clip_limit=0.01, nbins=256)`` for a 2-D float64 plane and a scalar kernel size, as the project recalls it.  Everything but
one float32 interpolation is integer arithmetic; the device result equals this file bit for bit.  Parity with skimage
itself is unpinned: every convention below is recalled, not pinned by an installed skimage, and ``RECALLED_CLAHE`` names
each one.

``branch_counts`` repeats ``clip_histogram`` with a counter per branch; the fixture's generator uses it to show that the
file as a whole reaches every one of them."""
import numpy as np
import scipy.ndimage

from tests import fiber_markers_reference as fmr
from tests import frangi_reference as fr

NR = 2 ** 14
NBINS = 256
CLIP_LIMIT = 0.01

# Every recalled convention of the statement, by name.  "doubt" notes where the project's own recollection is less firm;
# the text of the statement is the contract either way.
RECALLED_CLAHE = {
    "grey_levels": "the plane is rescaled to 2^14 grey levels, 0 .. 16383 (NR_OF_GRAY), whatever its input range",
    "bin_size": "bin = grey // (1 + NR // nbins): 65 for 256 bins, so only bins 0 .. 252 are ever occupied",
    "pad": "pad k // 2 before and (k - s % k) % k + ceil(k / 2) after each axis, mode='reflect' (the border pixel is not "
           "repeated); the padded sides are multiples of k",
    "tile_origin": "histogram tile t of an axis covers the original indices [t k, (t + 1) k): the tiles start k // 2 into "
                   "the padded plane, at the plane's own origin",
    "clim": "clim = int(clip(clip_limit * k * k, 1, None)) for clip_limit > 0, else NR (no clipping below 2^14 per bin)",
    "clip_phases": "clip_histogram: clip at clim and count the excess; add excess // nbins to every bin below clim - that "
                   "and lift the bins between up to clim (measured on the updated counts); then the strided one-by-one "
                   "loop with step max(1, under // excess), the early break at excess <= 0 (it may go below 0) and the "
                   "no-progress break",
    "map_scale": "map = int(min(cumsum(hist) as float64 * ((NR - 1) / (k * k)), NR - 1)): one float64 product, truncated",
    "map_pad": "the tile maps are padded by one tile on every side, mode='edge'",
    "coefficients": "a pixel at offset j of its block weighs the next tile by j / k and the previous one by 1 - j / k, per "
                    "axis, in float64; doubt: whether skimage forms (k - j) / k in place of 1 - j / k",
    "corner_order": "the four terms are float32(map * coefficient product), added in float32 in the order (0,0), (0,1), "
                    "(1,0), (1,1)",
    "truncation": "the float32 sum is truncated to uint16",
    "rescales": "rescale_intensity(in_range='image') before (to 0 .. NR - 1) and after (to 0 .. 1): clip to [min, max], "
                "(x - min) / (max - min) * (omax - omin) + omin; a constant plane is clipped to [omin, omax] instead; "
                "doubt: the constant-plane rule",
    "round": "np.round (half to even) before the cast to uint16",
}


def rescale(img, omin, omax):                 # rescale_intensity(in_range='image')
    imin, imax = img.min(), img.max()
    img = np.clip(img, imin, imax)
    if imin != imax:
        img = (img - imin) / (imax - imin)
        return img * (omax - omin) + omin
    return np.clip(img, omin, omax)           # RECALLED: the constant-plane rule


def clip_histogram(hist, clip_limit):         # hist: int64[nbins], modified in place
    excess_mask = hist > clip_limit
    excess = hist[excess_mask]
    n_excess = excess.sum() - excess.size * clip_limit
    hist[excess_mask] = clip_limit
    bin_incr = n_excess // hist.size
    upper = clip_limit - bin_incr
    low_mask = hist < upper
    n_excess -= hist[low_mask].size * bin_incr
    hist[low_mask] += bin_incr
    mid_mask = np.logical_and(hist >= upper, hist < clip_limit)
    mid = hist[mid_mask]
    n_excess += mid.sum() - mid.size * clip_limit
    hist[mid_mask] = clip_limit
    while n_excess > 0:
        prev_n_excess = n_excess
        for index in range(hist.size):
            under_mask = hist < clip_limit
            step_size = max(1, np.count_nonzero(under_mask) // n_excess)
            under_mask = under_mask[index::step_size]
            hist[index::step_size][under_mask] += 1
            n_excess -= np.count_nonzero(under_mask)      # may go below 0
            if n_excess <= 0:
                break
        if prev_n_excess == n_excess:
            break
    return hist


def map_histogram(hist, min_val, max_val, n_pixels):
    out = np.cumsum(hist, axis=-1).astype(float)
    out *= (max_val - min_val) / n_pixels
    out += min_val
    np.clip(out, a_min=None, a_max=max_val, out=out)
    return out.astype(int)                                # truncation


def tile_histograms(gray, k, nbins=NBINS):
    """(img, ps, nh, hist): the padded, binned plane, the leading pad, the tile counts per axis and the int64 histograms
    [nh[0] * nh[1], nbins] of the statement, before clipping."""
    H, W = gray.shape
    ps = k // 2
    pe = [(k - s % k) % k + int(np.ceil(k / 2.)) for s in (H, W)]
    img = np.pad(gray, [[ps, pe[0]], [ps, pe[1]]], mode='reflect')
    bin_size = 1 + NR // nbins                            # 65 for 256 bins: values 0 .. 252
    img = (np.arange(NR, dtype=np.uint16) // bin_size)[img]
    nh = [int(s / k) - 1 for s in img.shape]              # == ceil(H / k), ceil(W / k)
    tiles = img[ps:ps + nh[0] * k, ps:ps + nh[1] * k].reshape(nh[0], k, nh[1], k) \
        .transpose(0, 2, 1, 3).reshape(nh[0] * nh[1], k * k)
    hist = np.apply_along_axis(np.bincount, -1, tiles, minlength=nbins)
    return img, ps, nh, hist


def clip_limit_count(k, clip_limit):
    ke = k * k
    return int(np.clip(clip_limit * ke, 1, None)) if clip_limit > 0.0 else NR


def clahe(gray, k, clip_limit, nbins):        # gray: uint16 [H, W] in 0 .. NR-1; k: int
    H, W = gray.shape
    img, ps, nh, hist = tile_histograms(gray, k, nbins)
    ke = k * k
    clim = clip_limit_count(k, clip_limit)
    hist = np.apply_along_axis(clip_histogram, -1, hist, clip_limit=clim)
    maps = map_histogram(hist, 0, NR - 1, ke).reshape(nh[0], nh[1], nbins)
    map_array = np.pad(maps, [[1, 1], [1, 1], [0, 0]], mode='edge')
    npr = [int(s / k) for s in img.shape]
    blocks = img.reshape(npr[0], k, npr[1], k).transpose(0, 2, 1, 3).reshape(npr[0] * npr[1], ke)
    cr = np.repeat(np.arange(k) / k, k)                   # row coefficient of each block pixel
    cc = np.tile(np.arange(k) / k, k)                     # column coefficient
    result = np.zeros(blocks.shape, dtype=np.float32)
    for er, ec in ((0, 0), (0, 1), (1, 0), (1, 1)):       # this order
        em = map_array[er:er + npr[0], ec:ec + npr[1]].reshape(npr[0] * npr[1], nbins)
        mapped = np.take_along_axis(em, blocks, axis=-1)
        coeff = (cr if er else 1 - cr) * (cc if ec else 1 - cc)        # float64
        result += (mapped * coeff).astype(np.float32)     # float64 product, narrowed, added in float32
    result = result.astype(np.uint16)                     # truncation
    result = result.reshape(npr[0], npr[1], k, k).transpose(0, 2, 1, 3).reshape(img.shape)
    return result[ps:ps + H, ps:ps + W], maps


def equalize_adapthist(x, kernel_size, clip_limit=CLIP_LIMIT, nbins=NBINS):
    """(result float64 in [0, 1], gray uint16, maps int [nty, ntx, nbins], raw uint16)."""
    gray = np.round(rescale(np.asarray(x, float), 0, NR - 1)).astype(np.uint16)    # half to even
    raw, maps = clahe(gray, int(kernel_size), clip_limit, nbins)
    return rescale(raw.astype(float), 0.0, 1.0), gray, maps, raw


def contrast_adjust(channel, blur=2, kernel_size=8, clip_limit=CLIP_LIMIT):      # the front of segment_fibers
    b = scipy.ndimage.gaussian_filter(np.asarray(channel, float), sigma=blur)
    return equalize_adapthist(b / np.max(b), kernel_size, clip_limit)


def contrast_device(channel, blur, kernel_size, clip_limit):
    """The statement with the signature of fiber_segmentation._contrast_device."""
    return contrast_adjust(channel, blur, kernel_size, clip_limit)[0]


def channel_watershed_inputs_device(channel, blur, kernel_size, sigmas, ridge_cutoff, sobel_blur, thresholds):
    """The statement with the signature of fiber_segmentation._channel_watershed_inputs_device."""
    contrast = contrast_adjust(channel, blur, kernel_size)[0]
    ridges = fr.frangi(contrast, sigmas, fr.BETA, fr.GAMMA, fr.SCALE)
    return (contrast, ridges) + tuple(fmr.watershed_inputs(ridges, ridge_cutoff, sobel_blur, thresholds))


# ---- the branches of clip_histogram ---------------------------------------------------------------------------------------
BRANCHES = ("no_excess", "excess", "bin_incr", "low", "mid", "loop", "loop_second_pass", "loop_all_indices", "step_above_one",
            "break_excess_spent", "excess_below_zero", "break_no_progress")


def branch_counts(hist, clim):
    """clip_histogram on a copy of one histogram, counting the branches it reaches: name -> 0 / 1."""
    hist = np.array(hist, dtype=np.int64)
    got = dict.fromkeys(BRANCHES, 0)
    excess_mask = hist > clim
    n_excess = hist[excess_mask].sum() - np.count_nonzero(excess_mask) * clim
    got["excess" if excess_mask.any() else "no_excess"] = 1
    hist[excess_mask] = clim
    bin_incr = n_excess // hist.size
    got["bin_incr"] = int(bin_incr > 0)
    upper = clim - bin_incr
    low_mask = hist < upper
    got["low"] = int(bin_incr > 0 and low_mask.any())
    n_excess -= np.count_nonzero(low_mask) * bin_incr
    hist[low_mask] += bin_incr
    mid_mask = np.logical_and(hist >= upper, hist < clim)
    got["mid"] = int(mid_mask.any())
    n_excess += hist[mid_mask].sum() - np.count_nonzero(mid_mask) * clim
    hist[mid_mask] = clim
    passes = 0
    while n_excess > 0:
        got["loop"] = 1
        passes += 1
        got["loop_second_pass"] |= int(passes > 1)
        prev = n_excess
        for index in range(hist.size):
            under = hist < clim
            step = max(1, np.count_nonzero(under) // n_excess)
            got["step_above_one"] |= int(step > 1)
            under = under[index::step]
            hist[index::step][under] += 1
            n_excess -= np.count_nonzero(under)
            if n_excess <= 0:
                got["break_excess_spent"] = 1
                got["excess_below_zero"] |= int(n_excess < 0)
                break
        else:
            got["loop_all_indices"] = 1
        if prev == n_excess:
            got["break_no_progress"] = 1
            break
    return got, hist


def tile_branches(gray, k, clip_limit):
    """name -> the number of tiles of this case that reach the branch; also checks branch_counts against clip_histogram."""
    _, _, _, hist = tile_histograms(gray, k)
    clim = clip_limit_count(k, clip_limit)
    total = dict.fromkeys(BRANCHES, 0)
    for row in hist:
        got, clipped = branch_counts(row, clim)
        assert np.array_equal(clipped, clip_histogram(row.astype(np.int64).copy(), clim))
        for name, n in got.items():
            total[name] += n
    return total


# ---- planes ---------------------------------------------------------------------------------------------------------------
def noisy_bars(h, w, seed, period=6, noise=0.3):
    """Bright bars of the given period across the columns, with even noise."""
    rs = np.random.RandomState(seed)
    return ((np.arange(w) // (period // 2)) % 2)[None, :] * 1.0 + noise * rs.random_sample((h, w))


def smooth(h, w):
    """A smooth pattern: a product of two slow waves, no noise."""
    yy, xx = np.mgrid[:h, :w]
    return 2.0 + np.sin(yy / 9.0) * np.cos(xx / 7.0)


def single_pixel(h, w):
    out = np.zeros((h, w))
    out[h // 2, w // 3] = 1.0
    return out


def patterns(h, w, seed=None):
    """name -> float64 [h, w] plane: the fixture's pattern classes at any size."""
    seed = 1000 * h + w if seed is None else seed
    rs = np.random.RandomState(seed)
    return {"bars": noisy_bars(h, w, seed), "smooth": smooth(h, w), "noise": rs.random_sample((h, w)) * 40.0,
            "constant": np.full((h, w), 0.75), "single_pixel": single_pixel(h, w), "fibres": fr.bars(h, w, rs, 4)}


def front(channel, blur=2):
    """The blurred channel over its maximum: what the statement's contrast_adjust hands to equalize_adapthist."""
    b = scipy.ndimage.gaussian_filter(np.asarray(channel, float), sigma=blur)
    return b / np.max(b)


def fixture_channels():
    """name -> (raw channel, k, clip_limit) of the g30 fixture (tests/golden/make_golden_clahe.py), in its order."""
    return {
        "bars_k32": (noisy_bars(64, 64, 30), 32, 0.01),
        "smooth_k32_clim3": (smooth(64, 64), 32, 0.003),
        "bars_k32_noclip": (noisy_bars(64, 64, 30), 32, 0.0),
        "bars_16x16_k8": (noisy_bars(16, 16, 31), 8, 0.01),
        "noise_24x16_k8": (patterns(24, 16)["noise"], 8, 0.01),
        "fibres_40x24_k16": (patterns(40, 24)["fibres"], 16, 0.01),
        "bars_32x32_k16": (noisy_bars(32, 32, 32), 16, 0.01),
        "constant": (np.full((16, 16), 0.75), 8, 0.01),
        "single_pixel": (single_pixel(16, 16), 8, 0.01),
        "odd_33x31_k3": (patterns(33, 31)["fibres"], 3, 0.01),
        "odd_35x29_k5": (noisy_bars(35, 29, 33), 5, 0.01),
        "odd_40x90_k7": (patterns(40, 90)["fibres"], 7, 0.01),
        "k1_6x6": (patterns(6, 6)["noise"], 1, 0.01),
        "field_128_k8": (patterns(128, 128)["fibres"], 8, 0.01),
    }


def fixture_cases():
    """name -> (plane, k, clip_limit): every channel of fixture_channels() after the sigma = 2 blur and the division by the
    maximum, what the statement's contrast_adjust hands to equalize_adapthist."""
    return {name: (front(channel), k, clip_limit) for name, (channel, k, clip_limit) in fixture_channels().items()}


FULL_LIMIT = 1100                       # cases above this many pixels store digests of gray, maps and raw
CHAIN_CHANNEL = ("fibres", 32, 32, 27)  # the chained case: fr.bars at 32 x 32, seed 27, through contrast_adjust(blur=2, k=8)


def chain_channel():
    _, h, w, seed = CHAIN_CHANNEL
    return fr.bars(h, w, np.random.RandomState(seed), 5) * 200.0
