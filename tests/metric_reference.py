"""numpy reference of FlowSOM's distances (distf 1-4) for map_data_to_nodes and the online SOM loop.

Every array operation below is one IEEE binary64 operation per element, and the channel loop is written out, so each
(row, node) distance is the value of the C loop of include/pxsom.h (channels ascending, one rounding per operation, no
contraction).  The online loop restates oracle/pxsom_oracle.c orc_som_online_ex with the BMU distance as a parameter; its
`change` accumulator is summed sequentially (np.cumsum) in the C order of the (node, channel) terms.
"""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def distances(x, w, distf):
    """[n, K] distances of the rows x [n, C] to the nodes w [K, C] (both converted to binary64)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n, c = x.shape
    k = w.shape[0]
    with np.errstate(all="ignore"):
        if distf == 4:
            nom = np.zeros((n, k))
            d1 = np.zeros((n, 1))
            d2 = np.zeros((1, k))
            for j in range(c):
                xj, wj = x[:, j, None], w[None, :, j]
                nom = nom + xj * wj
                d1 = d1 + xj * xj
                d2 = d2 + wj * wj
            return (-nom / (np.sqrt(d1) * np.sqrt(d2))) + 1.0
        d = np.zeros((n, k))
        for j in range(c):
            t = x[:, j, None] - w[None, :, j]
            if distf == 1:
                d = d + np.abs(t)
            elif distf == 2:
                d = d + t * t
            elif distf == 3:
                t = np.abs(t)
                d = np.where(t > d, t, d)   # a NaN t never compares greater: the channel is skipped
            else:
                raise ValueError("distf %r" % (distf,))
        return np.sqrt(d) if distf == 2 else d


def map_data_to_nodes(nodes, data, distf, chunk=1 << 16):
    """(labels int32, 1-based; dists float64): first strict minimum below DBL_MAX over nodes ascending; label 0 and
    DBL_MAX when no distance compares smaller (NaN included)."""
    data = np.asarray(data, dtype=np.float64)
    n = data.shape[0]
    labels = np.zeros(n, dtype=np.int32)
    dists = np.full(n, DBL_MAX)
    for a in range(0, n, chunk):
        d = distances(data[a:a + chunk], nodes, distf)
        best = np.full(d.shape[0], DBL_MAX)
        lab = np.zeros(d.shape[0], dtype=np.int32)
        for cd in range(d.shape[1]):
            upd = d[:, cd] < best
            best = np.where(upd, d[:, cd], best)
            lab = np.where(upd, cd + 1, lab)
        labels[a:a + chunk] = lab
        dists[a:a + chunk] = best
    return labels, dists


def online_nearest(d):
    """FlowSOM's online BMU: nearest = 0; for cd: if d[cd] < d[nearest]: nearest = cd."""
    nearest = 0
    for cd in range(1, len(d)):
        if d[cd] < d[nearest]:
            nearest = cd
    return nearest


def _nhbrdist(xdim, ydim):
    gx, gy = np.divmod(np.arange(xdim * ydim), ydim)
    return np.maximum(np.abs(gx[:, None] - gx[None, :]), np.abs(gy[:, None] - gy[None, :])).astype(np.float64)


def som_online(data, codes, xdim, ydim, rlen, alpha_range, radius_range, order, distf, int_abs=False):
    """Trained codebook [K, C]: the loop of orc_som_online_ex with FlowSOM's distance `distf`."""
    data = np.asarray(data, dtype=np.float64)
    codes = np.array(codes, dtype=np.float64, copy=True)
    n = data.shape[0]
    k_nodes = codes.shape[0]
    assert k_nodes == xdim * ydim
    nhb = _nhbrdist(xdim, ydim)
    a0, a1 = float(alpha_range[0]), float(alpha_range[1])
    r0, r1 = float(radius_range[0]), float(radius_range[1])
    niter = rlen * n
    threshold = r0
    threshold_step = (r0 - r1) / float(niter)
    change = 1.0
    k = 0
    steps = 0
    while k < niter:
        if k % n == 0:
            if change < 1:
                k = niter   # the body still runs once with k == niter, then the loop ends
            change = 0.0
        xi = data[order[steps]]
        nearest = online_nearest(distances(xi[None, :], codes, distf)[0])
        if threshold < 1.0:
            threshold = 0.5
        alpha = a0 - (a0 - a1) * float(k) / float(niter)
        sel = np.flatnonzero(~(nhb[nearest] > threshold))
        tmp = xi[None, :] - codes[sel]
        if int_abs:
            with np.errstate(invalid="ignore"):
                small = np.abs(tmp) < 2147483648.0
                terms = np.where(small, np.abs(np.trunc(np.where(small, tmp, 0.0))), np.abs(tmp))
        else:
            terms = np.abs(tmp)
        change = float(np.cumsum(np.concatenate([[change], terms.ravel()]))[-1])
        codes[sel] = codes[sel] + tmp * alpha
        threshold -= threshold_step
        steps += 1
        k += 1
    return codes
