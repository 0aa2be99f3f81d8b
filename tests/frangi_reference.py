"""The numpy / scipy statement of K26 (include/pxsom.h "K26"): skimage 0.19's ``frangi(x, sigmas, beta=0.5, gamma=15,
black_ridges=False, mode="reflect")`` for a 2-D image, as the project recalls it -- ``hessian_matrix`` is K22's statement
(tests/projection_mask_reference.hessian: np.gradient twice on the reflect-mode blur, times sigma squared), the eigenvalues
are ordered by magnitude under K22's tie rule, ``alpha`` only enters the 3-D formula.  Parity with skimage itself is
unpinned.

``exp_neg`` is the contract's own exponential for t <= 0, in plain binary64 operations that numpy performs one by one (no
fused multiply-add) and that the kernel repeats without contraction: the device result equals this file bit for bit."""
import numpy as np
from scipy import ndimage as ndi

from tests import fiber_markers_reference as fmr
from tests import projection_mask_reference as pmr

TOO_SMALL = pmr.TOO_SMALL
SIGMAS = (1, 3, 5, 7, 9)                # the reference's fiber_widths, range(1, 10, 2)
BETA, GAMMA, SCALE = 0.5, 15, 10000     # skimage 0.19's defaults and the reference's factor

LOG2E, LN2_HI, LN2_LO = 1.4426950408889634, 0.6931471803691238, 1.9082149292705877e-10
EXP_NEG_FLOOR = -708.0
INV_FACTORIAL = (1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333, 0.001388888888888889,
                 0.0001984126984126984, 2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07,
                 2.505210838544172e-08, 2.08767569878681e-09, 1.6059043836821613e-10)        # 1 / k!, k = 0 .. 13


def exp_neg(t):
    """exp(t) for t <= 0: 0 below -708 (no subnormal is ever produced), NaN for NaN, else k = rint(t * LOG2E),
    r = (t - k * LN2_HI) - k * LN2_LO, the degree-13 Taylor polynomial of exp(r) by Horner, times 2^k from its bits."""
    t = np.asarray(t, dtype=np.float64)
    in_range = t >= EXP_NEG_FLOOR                              # False for NaN
    ts = np.where(in_range, t, 0.0)
    k = np.rint(ts * LOG2E)
    r = (ts - k * LN2_HI) - k * LN2_LO
    p = np.full(t.shape, INV_FACTORIAL[13])
    for c in INV_FACTORIAL[12::-1]:
        p = p * r + c
    two_k = ((k.astype(np.int64) + 1023) << 52).view(np.float64)
    return np.where(np.isnan(t), np.nan, np.where(in_range, p * two_k, 0.0))


def np_exp(t):
    return np.exp(t)


def vesselness(x, sigma, bsq, gsq, exp=exp_neg):
    """One scale of the statement on a float64 [H, W] plane."""
    g = ndi.gaussian_filter(x, sigma, mode="reflect", truncate=4.0)
    g0, g1 = np.gradient(g, axis=0), np.gradient(g, axis=1)
    s2 = float(sigma) ** 2
    hrr, hrc, hcc = s2 * np.gradient(g0, axis=0), s2 * np.gradient(g0, axis=1), s2 * np.gradient(g1, axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = hrr - hcc
        r = np.sqrt(d * d + 4.0 * (hrc * hrc))
        t = hrr + hcc
        e_hi, e_lo = (t + r) / 2.0, (t - r) / 2.0
        lo_big = np.abs(e_lo) >= np.abs(e_hi)                  # K22's order and tie rule
        big, small = np.where(lo_big, e_lo, e_hi), np.where(lo_big, e_hi, e_lo)
        den = np.abs(big)
        den = np.where(den == 0, 1e-10, den)                   # skimage's _divide_nonzero
        q = small / den
        rb = q * q
        rg = small * small + big * big
        v = exp(-rb / bsq) * (1.0 - exp(-rg / gsq))            # divisions, not reciprocal multiplies
        return np.where(big > 0, 0.0, v)                       # "remove background"


def stages(x, sigmas=SIGMAS, beta=BETA, gamma=GAMMA, scale=SCALE, exp=exp_neg):
    """{"scales": [n, H, W] per-scale vesselness, "folded": their NaN-propagating maximum from zeros, "ridges": folded *
    scale}."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or min(x.shape) < 2:
        raise ValueError(TOO_SMALL)
    bsq, gsq = 2.0 * beta * beta, 2.0 * gamma * gamma
    out = np.zeros(x.shape)
    scales = []
    for sigma in sigmas:
        v = vesselness(x, sigma, bsq, gsq, exp)
        scales.append(v)
        out = np.maximum(out, v)
    return {"scales": np.array(scales), "folded": out, "ridges": out * float(scale)}


def frangi(x, sigmas=SIGMAS, beta=BETA, gamma=GAMMA, scale=1.0):
    return stages(x, sigmas, beta, gamma, scale)["ridges"]


def frangi_device(image, sigmas, beta, gamma, scale):
    """The statement with the signature of fiber_segmentation._frangi_device."""
    return frangi(image, sigmas, beta, gamma, scale)


def ridge_watershed_inputs_device(contrast, sigmas, ridge_cutoff, sobel_blur, thresholds):
    """The statement with the signature of fiber_segmentation._ridge_watershed_inputs_device."""
    ridges = frangi(contrast, sigmas, BETA, GAMMA, SCALE)
    return (ridges,) + tuple(fmr.watershed_inputs(ridges, ridge_cutoff, sobel_blur, thresholds))


def exp_neg_grid():
    """The arguments on which the gap of exp_neg to np.exp is measured: an even grid over [-708, 0], the same grid moved by
    an irrational step, and the multiples of ln2 / 2 (the ends of the reduced range)."""
    even = np.linspace(-708.0, 0.0, 200001)
    moved = np.clip(even + np.sqrt(2.0) * 1e-3, -708.0, 0.0)
    ends = -np.arange(0, 2043) * (np.log(2.0) / 2.0)
    return np.concatenate([even, moved, ends[ends >= -708.0], np.nextafter(ends[ends >= -708.0], 0.0)])


def exp_neg_gap(t):
    """The largest relative gap of exp_neg to np.exp over t, in units of 2^-53."""
    want = np.exp(t)
    return float(np.max(np.abs(exp_neg(t) - want) / want) * 2.0 ** 53)


# ---- planes ---------------------------------------------------------------------------------------------------------------
def bars(h, w, rs, n=5, noise=0.05):
    """n bright bars of half-width 1 - 4 in random directions on a dark plane, with even noise: values in [0, 1 + noise]."""
    yy, xx = np.mgrid[:h, :w]
    out = np.zeros((h, w))
    for _ in range(n):
        theta = rs.uniform(0, np.pi)
        cy, cx = rs.uniform(0, h), rs.uniform(0, w)
        half = rs.randint(1, 5)
        out[np.abs((yy - cy) * np.cos(theta) - (xx - cx) * np.sin(theta)) <= half] = 1.0
    return out + noise * rs.random_sample((h, w))


def dark_bars(bright, noise=0.05):
    """The same bars dark on bright.  Along a dark bar the larger eigenvalue is positive and the response 0, but its bright
    shoulders curve downwards across the bar and respond: the plane is not all zero, only darker where `bright` is bright."""
    return (1.0 + noise) - bright


def disc(h, w):
    yy, xx = np.mgrid[:h, :w]
    return ((yy - 0.45 * h) ** 2 + (xx - 0.55 * w) ** 2 <= (0.3 * min(h, w)) ** 2).astype(np.float64)


def ramp(h, w):
    return np.add.outer(np.arange(h) * 0.25, np.arange(w) * 0.125)


def patterns(h, w, seed=None):
    """name -> float64 [h, w] plane: the fixture's pattern classes at any size with h, w >= 2."""
    rs = np.random.RandomState(1000 * h + w if seed is None else seed)
    bright = bars(h, w, rs, 4)
    out = {"bars": bright, "dark_bars": dark_bars(bright), "disc": disc(h, w), "constant": np.full((h, w), 0.75),
           "ramp": ramp(h, w), "single_pixel": pmr.single_pixel(h, w, h // 2, w // 3).astype(np.float64),
           "quadrant": pmr.quadrant(h, w, (h + 1) // 2, (w + 1) // 2).astype(np.float64)}
    out["bars_1e6"] = out["bars"] * 1e6
    return out


def fixture_planes():
    """name -> plane of the g29 fixture (tests/golden/make_golden_frangi.py), in its order."""
    small = patterns(28, 28, seed=29)
    return {"bars": small["bars"], "dark_bars": small["dark_bars"], "disc": disc(24, 24), "constant": np.full((16, 16), 0.75),
            "ramp": ramp(16, 17), "single_pixel": patterns(16, 16)["single_pixel"], "quadrant": patterns(17, 16)["quadrant"],
            "bars_1e6": small["bars_1e6"], "wide": bars(40, 90, np.random.RandomState(30), 6),
            "tall": bars(90, 40, np.random.RandomState(31), 6)}
