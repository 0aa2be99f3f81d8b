"""The numpy + scipy statement of the K22 contract (include/pxsom.h "K22"): where skimage 0.19's Meijering ridge filter is
positive on a binary plane, and the ``object_mask`` chain with that stage between the hole fill and the labelling
("projection" objects), composed from tests/object_mask_reference.py.  The CPU tests check it against the g25 fixtures
(made by the reference's own ``_create_object_mask(..., "projection")`` over a restated ``filters.meijering`` that goes
through ``np.linalg.eigvalsh``); the GPU tests compare the device entry with it exactly."""
import numpy as np
import scipy.ndimage as ndi

from tests import object_mask_reference as omr

SIGMAS = (1, 2, 3, 4)           # the reference's range(1, 5, 1)
ALPHA = 0.5                     # skimage's default: 1 / ndim
TOO_SMALL = "Shape of array too small to calculate a numerical gradient"


def hessian(x, sigma):
    """(Hrr, Hrc, Hcc) of skimage 0.19's hessian_matrix: np.gradient twice on the reflect-mode blur, times sigma squared."""
    g = ndi.gaussian_filter(x, sigma, mode="reflect", truncate=4.0)
    g0, g1 = np.gradient(g, axis=0), np.gradient(g, axis=1)
    s2 = float(sigma ** 2)
    return s2 * np.gradient(g0, axis=0), s2 * np.gradient(g0, axis=1), s2 * np.gradient(g1, axis=1)


def ridge_sign(fg, sigmas=SIGMAS, alpha=ALPHA):
    """uint8 [H, W]: 1 where the filter's response is positive at some scale."""
    x = (np.asarray(fg) != 0).astype(np.float64)
    on = np.zeros(x.shape, dtype=bool)
    for sigma in sigmas:
        hrr, hrc, hcc = hessian(x, sigma)
        d = hrr - hcc
        r = np.sqrt(d * d + 4.0 * (hrc * hrc))
        t = hrr + hcc
        e_hi, e_lo = (t + r) / 2.0, (t - r) / 2.0
        lo_big = np.abs(e_lo) >= np.abs(e_hi)
        big, small = np.where(lo_big, e_lo, e_hi), np.where(lo_big, e_hi, e_lo)
        on |= (big + alpha * small) < 0
    return on.astype(np.uint8)


def object_mask(img, sigma, thresh, hole_size, min_area, max_area, local_block=None, ridge=None):
    """tests/object_mask_reference.object_mask with the ridge stage: ``ridge`` None or ``(sigmas, alpha)``."""
    x = omr.as_float_plane(img)
    blurred = x if sigma is None else omr.blur(x, sigma, "nearest")
    fg = omr.foreground(blurred, thresh, local_block).astype(np.uint8)
    if hole_size is not None:
        fg = omr.fill_holes(fg, hole_size)
    if ridge is not None:
        fg = ridge_sign(fg, ridge[0], ridge[1])
    labels, _, areas = omr.label_components(fg, 2)
    return omr.keep_by_area(labels, areas, min_area, max_area)


def create_projection_mask(img, sigma=1, thresh=None, hole_size="auto", fov_dim=400, min_object_area=10, max_object_area=100000):
    """_create_object_mask for "projection" objects, the "auto" sizes resolved as the reference resolves them."""
    h = np.asarray(img).shape[0]
    block = omr.get_block_size("local_thresh", fov_dim, h) if isinstance(thresh, str) else None
    if isinstance(hole_size, str):
        hole_size = omr.get_block_size("small_holes", fov_dim, h)
    return object_mask(img, sigma, thresh, hole_size, min_object_area, max_object_area, block, ridge=(SIGMAS, ALPHA))


# ---- patterns for the ridge tests ---------------------------------------------------------------------------------------
def single_pixel(h, w, y, x):
    m = np.zeros((h, w), dtype=np.uint8)
    m[y, x] = 1
    return m


def quadrant(h, w, cy, cx):
    """Ones above and left of (cy, cx): the corner where the two eigenvalues tie in magnitude."""
    m = np.zeros((h, w), dtype=np.uint8)
    m[:cy, :cx] = 1
    return m


def lines(h, w, rs, n=6):
    """Straight segments of width 1 - 3 in random directions."""
    m = np.zeros((h, w), dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w]
    for _ in range(n):
        cy, cx, ang, half = rs.uniform(0, h), rs.uniform(0, w), rs.uniform(0, np.pi), rs.randint(1, 4) / 2.0
        dist = np.abs((yy - cy) * np.cos(ang) - (xx - cx) * np.sin(ang))
        along = np.abs((yy - cy) * np.sin(ang) + (xx - cx) * np.cos(ang))
        m[(dist <= half) & (along <= 0.4 * max(h, w))] = 1
    return m


def discs(h, w, rs, n=5):
    m = np.zeros((h, w), dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w]
    for _ in range(n):
        cy, cx, r = rs.uniform(0, h), rs.uniform(0, w), rs.uniform(1.5, 0.2 * max(h, w) + 2)
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    return m


def ring(h, w):
    yy, xx = np.mgrid[:h, :w]
    d2 = (yy - h / 2.0) ** 2 + (xx - w / 2.0) ** 2
    r = 0.35 * min(h, w)
    return ((d2 <= r * r) & (d2 >= (r - 2.5) ** 2)).astype(np.uint8)


def noise(h, w, rs, p=0.3):
    return (rs.rand(h, w) < p).astype(np.uint8)
