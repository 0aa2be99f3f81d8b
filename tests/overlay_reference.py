"""The numpy statement of K29 (include/pxsom.h "K29"): the overlay of ``plot_utils.create_overlay`` (inner borders,
skimage 0.19's ``rescale_intensity`` as recalled, the white and red compositing), the channel sums of
``generate_deepcell_input`` and the colour gather of ``save_colored_masks``.  Test infrastructure: the GPU tests compare the
device with it, array_equal, and the CPU tests pin it to tests/golden/g32_overlays.npz, which holds the outputs of the
reference's own functions.

scikit-image is not in this image.  Every detail of it that is taken from memory sits behind a switch of
``RECALLED_OVERLAY``; tests/test_overlays.py shows what each switch changes."""
import numpy as np

RECALLED_OVERLAY = {
    # rescale_intensity clips the image to in_range BEFORE it scales (otherwise: scale, then clip to the output range)
    "clip_then_scale": True,
    # in_range lo == hi: no division, the clipped image is clipped again to the output range and cast
    # (otherwise: such a channel is left at zero)
    "equal_range_branch": True,
    # the result becomes uint8 by numpy's cast, which truncates (otherwise: rounds to nearest)
    "truncating_cast": True,
}

_OFFSETS4 = ((-1, 0), (1, 0), (0, -1), (0, 1))


def inner_boundaries(seg):
    """find_boundaries(seg, connectivity=1, mode="inner") as tests/cell_mask_reference.py states it: a 4-neighbour inside
    the image holds another label (compared in the image's dtype; the edge padding never adds one) and the pixel's own
    label is not the background 0."""
    seg = np.asarray(seg)
    h, w = seg.shape
    pad = np.pad(seg, 1, mode="edge")
    edge = np.zeros(seg.shape, dtype=bool)
    for dy, dx in _OFFSETS4:
        edge |= pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] != seg
    return edge & (seg != 0)


def borders(seg):
    """The ``<fov>_segmentation_borders.tiff`` plane: uint8, 255 on an inner border pixel."""
    out = inner_boundaries(seg).astype(np.uint8)
    out[out > 0] = 255
    return out


def rescale_intensity_uint8(image, lo, hi, recalled=None):
    """rescale_intensity(image, in_range=(lo, hi), out_range="uint8") with Python floats ``lo <= hi``, in numpy's own
    arithmetic for the image's dtype (binary32 for float32, binary64 for the integer dtypes)."""
    r = dict(RECALLED_OVERLAY, **(recalled or {}))
    lo, hi = float(lo), float(hi)
    omin, omax = 0.0, 255.0

    def cast(x):
        return (x if r["truncating_cast"] else np.rint(x)).astype(np.uint8)

    if lo == hi:
        if not r["equal_range_branch"]:
            return np.zeros(image.shape, dtype=np.uint8)
        return cast(np.clip(np.clip(image, lo, hi), omin, omax))
    if r["clip_then_scale"]:
        image = np.clip(image, lo, hi)
        image = (image - lo) / (hi - lo)
        return cast(image * (omax - omin) + omin)
    image = (image - lo) / (hi - lo)
    return cast(np.clip(image * (omax - omin) + omin, omin, omax))


def percentiles_positive(plane, q=(5, 95)):
    return np.percentile(plane[plane > 0], list(q))


def percentile_listq_f32(values, q):
    """np.percentile(values, [q...]) of a float32 vector, restated with the arithmetic numpy 2 uses for a list of q: index
    and fraction in binary64, ``b - a`` in binary32, the interpolation in binary64."""
    v = np.sort(np.asarray(values, dtype=np.float32))
    out = []
    for one in q:
        vi = (np.float64(one) / 100) * np.float64(v.size - 1)
        lo = int(np.floor(vi))
        hi = min(lo + 1, v.size - 1)
        g = vi - lo
        a, b = v[lo], v[hi]
        d = np.float64(np.float32(b - a))
        out.append(np.float64(b) - d * (1.0 - g) if g >= 0.5 else np.float64(a) + d * g)
    return np.array(out, dtype=np.float64)


def tif_overlay_preprocess(plotting_tif):
    """[H, W] -> blue; channel i of [H, W, c] -> byte 2 - i."""
    plotting_tif = np.asarray(plotting_tif)
    out = np.zeros(plotting_tif.shape[:2] + (3,), dtype=plotting_tif.dtype)
    if plotting_tif.ndim == 2:
        out[..., 2] = plotting_tif
        return out
    out[..., :plotting_tif.shape[2]] = plotting_tif
    return np.flip(out, axis=2)


OVERLAY_ZERO, OVERLAY_RESCALE, OVERLAY_CLIP = 0, 1, 2      # include/pxsom.h PXSOM_OVERLAY_*


def compose(planes, modes, ranges, seg, alt=None, recalled=None):
    """pxsom_overlay_rgb as include/pxsom.h states it: output byte j (red, green, blue) is 0 under mode OVERLAY_ZERO
    (``planes[j]`` may be None), else rescale_intensity of ``planes[j]`` over ``ranges[j] = (lo, hi)`` -- OVERLAY_RESCALE
    with lo < hi, OVERLAY_CLIP with lo == hi; then the white border of ``seg`` and the red one of ``alt`` -> uint8
    [H, W, 3]."""
    seg = np.asarray(seg)
    out = np.zeros(seg.shape + (3,), dtype=np.uint8)
    for j in range(3):
        if modes[j] == OVERLAY_ZERO:
            continue
        lo, hi = ranges[j]
        assert (lo < hi) if modes[j] == OVERLAY_RESCALE else (modes[j] == OVERLAY_CLIP and lo == hi)
        out[:, :, j] = rescale_intensity_uint8(np.asarray(planes[j]), lo, hi, recalled)
    out[inner_boundaries(seg), :] = 255
    if alt is not None:
        edge = inner_boundaries(alt)
        out[edge, 0] = 255
        out[edge, 1:] = 0
    return out


def overlay(plotting_tif, seg, alt=None, recalled=None):
    """create_overlay from the arrays on: uint8 [H, W, 3].  A channel with a zero maximum stays zero; every other one is
    rescaled from the 5th .. 95th percentile of its positive pixels."""
    tif = tif_overlay_preprocess(plotting_tif)
    modes, ranges = [OVERLAY_ZERO] * 3, [(0.0, 0.0)] * 3
    for idx in range(3):
        plane = tif[:, :, idx]
        if np.max(plane) == 0:
            continue
        lo, hi = percentiles_positive(plane)
        modes[idx], ranges[idx] = (OVERLAY_CLIP if lo == hi else OVERLAY_RESCALE), (lo, hi)
    return compose([tif[:, :, idx] for idx in range(3)], modes, ranges, seg, alt, recalled)


def deepcell_pages(stack, nuc_idx, mem_idx):
    """The two pages of generate_deepcell_input from a C-contiguous [H, W, C] stack: np.sum over the listed channels,
    assigned into the stack's dtype (integers wrap); a page stays zero for an empty list."""
    stack = np.ascontiguousarray(stack)
    out = np.zeros((2,) + stack.shape[:2], dtype=stack.dtype)
    if len(nuc_idx):
        out[0] = np.sum(np.ascontiguousarray(stack[:, :, list(nuc_idx)]), axis=2)
    if len(mem_idx):
        out[1] = np.sum(np.ascontiguousarray(stack[:, :, list(mem_idx)]), axis=2)
    return out


def color_table(mc_colors):
    """The per-row conversion the host does once: (mc_colors * 255.999).astype(uint8)."""
    return (np.asarray(mc_colors, dtype=np.float64) * 255.999).astype(np.uint8)


def colored_mask(mask, mc_colors):
    """(mc_colors[mask] * 255.999).astype(np.uint8), as save_colored_masks writes it."""
    return (np.asarray(mc_colors)[np.asarray(mask)] * 255.999).astype(np.uint8)


# ---- inputs the tests and the generator share ---------------------------------------------------------------------
def cells(h, w, seed, dtype=np.int32, big=False):
    """A label plane with what the border test has to meet: rectangular cells touching the image edge, pairs adjacent
    without background, gaps of background, single-pixel cells; ``big``: labels above 2^15."""
    rs = np.random.RandomState(seed)
    seg = np.zeros((h, w), dtype=np.int64)
    ny, nx = max(1, h // 5), max(1, w // 6)
    ys = np.linspace(0, h, ny + 1).astype(int)
    xs = np.linspace(0, w, nx + 1).astype(int)
    lab = 1
    for i in range(ny):
        for j in range(nx):
            if rs.rand() < 0.2:
                continue
            y1 = ys[i + 1] - (1 if rs.rand() < 0.5 else 0)
            x1 = xs[j + 1] - (1 if rs.rand() < 0.5 else 0)
            seg[ys[i]:max(y1, ys[i] + 1), xs[j]:max(x1, xs[j] + 1)] = lab
            lab += 1
    for _ in range(max(1, h * w // 40)):
        seg[rs.randint(h), rs.randint(w)] = lab        # single-pixel cells
        lab += 1
    if big:
        seg[seg > 0] += 40000
    info = np.iinfo(dtype)
    if seg.max() > info.max:
        seg = np.where(seg > 0, (seg - 1) % info.max + 1, 0)
    return seg.astype(dtype)


def signal(h, w, seed, dtype, kind="plain"):
    """An image plane: ``plain`` random with zeros, values above the 95th percentile and (signed dtypes) negative ones;
    ``zero`` all zero; ``one`` a single positive pixel (the two percentiles coincide: the lo == hi branch); ``equal``
    every positive pixel the same."""
    rs = np.random.RandomState(seed)
    dtype = np.dtype(dtype)
    if kind == "zero":
        return np.zeros((h, w), dtype=dtype)
    if kind == "one":
        out = np.zeros((h, w), dtype=dtype)
        out[rs.randint(h), rs.randint(w)] = 77 if dtype.kind != "f" else 300.5
        return out
    if kind == "equal":
        return (rs.rand(h, w) < 0.6).astype(dtype) * dtype.type(9)
    if dtype.kind == "f":
        out = (rs.gamma(2.0, 3.0, size=(h, w)) * (rs.rand(h, w) < 0.8)).astype(np.float32)
        out[rs.rand(h, w) < 0.05] *= np.float32(-1.5)
        out[rs.rand(h, w) < 0.02] *= np.float32(40)
        return out
    top = min(np.iinfo(dtype).max, 3000)
    out = (rs.gamma(2.0, top / 12.0, size=(h, w)) * (rs.rand(h, w) < 0.8)).clip(0, top).astype(np.int64)
    if dtype.kind == "i":
        neg = rs.rand(h, w) < 0.05
        out[neg] = -out[neg]
    return out.astype(dtype)
