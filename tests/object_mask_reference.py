"""The numpy + scipy statement of the K16 contracts (include/pxsom.h "object masks"): labelling order, the hole fill,
the area filter, the three foreground predicates, the two blurs, and their chain (``object_mask``).  The CPU tests check
it against the g21 fixtures (made by the reference's own ``_create_object_mask`` / ``create_cell_mask``); the GPU tests
compare the device entries with it exactly."""
import numpy as np
import scipy.ndimage as ndi


def label_components(fg, connectivity, invert=False):
    """(labels int32, n, areas int64 [n + 1]) -- scipy numbers components by their first pixel in raster order."""
    on = (np.asarray(fg) != 0) ^ bool(invert)
    labels, n = ndi.label(on, structure=ndi.generate_binary_structure(2, connectivity))
    labels = labels.astype(np.int32)
    return labels, int(n), np.bincount(labels.ravel(), minlength=n + 1)


def fill_holes(fg, area_threshold):
    """morphology.remove_small_holes: background components (4-neighbourhood) of area < area_threshold become foreground."""
    on = np.asarray(fg) != 0
    holes, _, areas = label_components(on, 1, invert=True)
    return (on | ((holes != 0) & (areas[holes] < area_threshold))).astype(np.uint8)


def keep_by_area(labels, areas, min_area, max_area):
    """map_array(labels, all, all * keep): labels outside the area range become 0, none is renumbered."""
    areas = np.asarray(areas)
    keep = (areas >= min_area) & (areas <= max_area)
    keep[0] = False
    return np.where(keep[labels], labels, 0).astype(np.int32)


def blur(plane, sigma, mode):
    return ndi.gaussian_filter(plane, sigma, mode=mode, truncate=4.0)


def as_float_plane(img):
    """skimage's preserve_range conversion: float32 / float64 stay, anything else becomes float64."""
    img = np.asarray(img)
    return img if img.dtype in (np.float32, np.float64) else img.astype(np.float64)


def foreground(blurred, thresh, local_block=None):
    if thresh is None:
        return blurred > 0
    if isinstance(thresh, str):
        assert thresh == "auto"
        return blurred > blur(blurred, (local_block - 1) / 6.0, "reflect")
    nonzero = blurred[blurred != 0]
    with np.errstate(invalid="ignore"):
        p = np.percentile(nonzero, thresh) if nonzero.size else np.nan
        return ~(blurred < p) & (blurred > 0)


def object_mask(img, sigma, thresh, hole_size, min_area, max_area, local_block=None):
    x = as_float_plane(img)
    blurred = x if sigma is None else blur(x, sigma, "nearest")
    fg = foreground(blurred, thresh, local_block).astype(np.uint8)
    if hole_size is not None:
        fg = fill_holes(fg, hole_size)
    labels, _, areas = label_components(fg, 2)
    return keep_by_area(labels, areas, min_area, max_area)


def get_block_size(block_type, fov_dim, img_shape):
    pixel_size = fov_dim / img_shape
    if block_type == "small_holes":
        return round((np.pi * 5) ** 2 / pixel_size)
    area = round(10 / pixel_size)
    return area + 1 if area % 2 == 0 else area


def create_object_mask(img, sigma=1, thresh=None, hole_size="auto", fov_dim=400, min_object_area=10, max_object_area=100000):
    """_create_object_mask for "blob" objects, the "auto" sizes resolved as the reference resolves them."""
    h = np.asarray(img).shape[0]
    block = get_block_size("local_thresh", fov_dim, h) if isinstance(thresh, str) else None
    if isinstance(hole_size, str):
        hole_size = get_block_size("small_holes", fov_dim, h)
    return object_mask(img, sigma, thresh, hole_size, min_object_area, max_object_area, block)


def cell_mask(seg, labels, sigma=10, min_object_area=0, max_hole_area=1000):
    """create_cell_mask after the table lookup: the cells in ``labels`` -> 0 / 1 mask."""
    member = np.isin(seg, labels).astype(np.int32)
    out = object_mask(member, sigma, None, max_hole_area, min_object_area, member.shape[0] * member.shape[1])
    return (out > 0).astype(np.int32)


# ---- patterns for the labelling tests (T: the kernel's tile edge) ------------------------------------------------------
def spiral(h, w):
    """A one-pixel-wide path that winds inwards from the top-left corner, one background pixel between its turns."""
    m = np.zeros((h, w), dtype=np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1
    while True:
        for _ in range(2):      # straight on, or one right turn
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= ay < h and 0 <= ax < w and m[ay, ax]):
                y, x = ny, nx
                m[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            return m


def serpentine(h, w):
    """Full rows on every other line, joined alternately at the right and the left end: one long snake."""
    m = np.zeros((h, w), dtype=np.uint8)
    m[::2] = 1
    for i, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if i % 2 == 0 else 0] = 1
    return m


def checkerboard(h, w):
    yy, xx = np.mgrid[:h, :w]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def nested_rings(h, w, step=3):
    """Concentric one-pixel rectangles every ``step`` pixels: object in hole in object ..."""
    m = np.zeros((h, w), dtype=np.uint8)
    k = 0
    while 2 * k < min(h, w):
        m[k, k:w - k] = 1
        m[h - 1 - k, k:w - k] = 1
        m[k:h - k, k] = 1
        m[k:h - k, w - 1 - k] = 1
        k += step
    return m
