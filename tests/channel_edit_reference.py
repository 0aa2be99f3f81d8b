"""Test infrastructure for the channel edits (smooth_channels, filter_with_nuclear_mask): a writer of the TIFF pages
tifffile makes of an array (``skimage.io.imsave``), a restated tifffile-faithful reader of them, the scipy / numpy
stand-ins of the two device entry points, and the notebook-2 cohort (cells 20 -> 22 -> 26) the g16 fixtures record.
Nothing here is a product path."""
import json
import os
import struct
import zlib

import numpy as np

_KIND_CODE = {"u": 1, "i": 2, "f": 3}


def write_shaped(path, array, compress=False):
    """One classic little-endian TIFF page holding ``array`` (2-D, or 3-D with a leading axis of 1) with the JSON shape
    description tifffile writes (``{"shape": [...]}``), SampleFormat and BitsPerSample of the array's dtype (8-byte
    integers included), one strip, uncompressed or deflate (``compress``, what a zlib-compressing writer makes)."""
    array = np.asarray(array)
    page = array.reshape(array.shape[-2:])
    if array.ndim not in (2, 3) or array.size != page.size:
        raise ValueError("one page only")
    data = np.ascontiguousarray(page, dtype=page.dtype.newbyteorder("<")).tobytes()
    if compress:
        data = zlib.compress(data, 6)
    desc = json.dumps({"shape": list(array.shape)}).encode("ascii") + b"\0"
    h, w = page.shape
    tags = [(256, 4, 1, w), (257, 4, 1, h), (258, 3, 1, page.dtype.itemsize * 8), (259, 3, 1, 8 if compress else 1),
            (262, 3, 1, 1), (270, 2, len(desc), None), (273, 4, 1, None), (277, 3, 1, 1), (278, 4, 1, h),
            (279, 4, 1, len(data)), (339, 3, 1, _KIND_CODE[page.dtype.kind])]
    ifd_size = 2 + 12 * len(tags) + 4
    desc_at = 8 + ifd_size
    data_at = desc_at + len(desc)
    ifd = struct.pack("<H", len(tags))
    for tag, kind, n, value in tags:
        value = desc_at if tag == 270 else data_at if tag == 273 else value
        ifd += struct.pack("<HHI", tag, kind, n) + (struct.pack("<HH", value, 0) if kind == 3 else struct.pack("<I", value))
    with open(path, "wb") as f:
        f.write(b"II*\0" + struct.pack("<I", 8) + ifd + struct.pack("<I", 0) + desc + data)


def read_shaped(path):
    """tifffile.imread of a single-page file, restated: the page's samples in the dtype its SampleFormat and
    BitsPerSample name, reshaped to the JSON shape description when there is one (``(H, W)`` otherwise).  Uncompressed
    and deflate strips, one sample per pixel, no predictor."""
    with open(path, "rb") as f:
        raw = f.read()
    bo = "<" if raw[:2] == b"II" else ">"
    (first,) = struct.unpack(bo + "I", raw[4:8])
    (count,) = struct.unpack(bo + "H", raw[first:first + 2])
    tags = {}
    for i in range(count):
        at = first + 2 + 12 * i
        tag, kind, n = struct.unpack(bo + "HHI", raw[at:at + 8])
        code, size = {1: ("B", 1), 2: ("s", 1), 3: ("H", 2), 4: ("I", 4)}[kind]
        body = raw[at + 8:at + 12]
        if n * size > 4:
            (off,) = struct.unpack(bo + "I", body)
            body = raw[off:off + n * size]
        tags[tag] = body[:n] if code == "s" else struct.unpack(bo + code * n, body[:n * size])
    assert tags.get(277, (1,))[0] == 1 and tags.get(317, (1,))[0] == 1
    dtype = np.dtype(bo + {1: "u", 2: "i", 3: "f"}[tags.get(339, (1,))[0]] + str(tags[258][0] // 8))
    strips = [raw[o:o + n] for o, n in zip(tags[273], tags[279])]
    if tags.get(259, (1,))[0] != 1:
        strips = [zlib.decompress(s) for s in strips]
    h, w = tags[257][0], tags[256][0]
    arr = np.frombuffer(b"".join(strips), dtype=dtype)[:h * w].reshape(h, w).astype(dtype.newbyteorder("="))
    if 270 in tags:
        try:
            shape = json.loads(bytes(tags[270]).rstrip(b"\0").decode("ascii"))["shape"]
            arr = arr.reshape(shape)
        except (ValueError, KeyError):
            pass
    return arr


# ---- stand-ins of the device entry points (pixel_cluster_utils._blur_device / _zero_device) -------------------------
def blur_standin(planes, sigmas):
    import scipy.ndimage as ndimage
    return [ndimage.gaussian_filter(p, sigma=s) for p, s in zip(planes, sigmas)]


def zero_standin(img, seg, exclude):
    img = img.copy()
    img[seg > 0 if exclude else seg == 0] = 0
    return img


# ---- the notebook-2 cohort of g16_cohort ------------------------------------------------------------------------------
COHORT_FOVS = ["fov0", "fov1", "fov2"]
COHORT_CHANNELS = ["chan0", "chan1", "chanX", "chanY"]
COHORT_SHAPE = (26, 22)


def cohort_inputs():
    """float32 channel images, int32 whole-cell and int64 (1, H, W) nuclear segmentations of three FOVs."""
    rs = np.random.RandomState(1607)
    out = {}
    for fov in COHORT_FOVS:
        for ch in COHORT_CHANNELS:
            img = rs.gamma(0.5, 2.0, size=COHORT_SHAPE).astype(np.float32)
            img[rs.uniform(size=img.shape) < 0.35] = 0
            out[f"img_{fov}_{ch}"] = img
        out["wc_" + fov] = rs.randint(0, 9, size=COHORT_SHAPE).astype(np.int32)
        nuc = np.zeros((1,) + COHORT_SHAPE, dtype=np.int64)
        nuc[0, 3:11, 4:12] = 1
        nuc[0, 14:23, 9:19] = 2
        out["nuc_" + fov] = nuc
    return out


def write_cohort(td, g, write_channel):
    """The cohort's files under ``td``: tiffs/<fov>/TIFs/<chan>.tiff (``write_channel(path, image)``),
    seg/<fov>_whole_cell.tiff, seg/<fov>_nuclear.tiff (tifffile pages of the int64 (1, H, W) arrays)."""
    tiff_dir, seg_dir = os.path.join(td, "tiffs"), os.path.join(td, "seg")
    os.makedirs(seg_dir, exist_ok=True)
    for fov in COHORT_FOVS:
        os.makedirs(os.path.join(tiff_dir, fov, "TIFs"), exist_ok=True)
        for ch in COHORT_CHANNELS:
            write_channel(os.path.join(tiff_dir, fov, "TIFs", ch + ".tiff"), g[f"img_{fov}_{ch}"])
        write_shaped(os.path.join(seg_dir, fov + "_whole_cell.tiff"), g["wc_" + fov])
        write_shaped(os.path.join(seg_dir, fov + "_nuclear.tiff"), g["nuc_" + fov])
    return tiff_dir, seg_dir


def run_cohort(td, tiff_dir, seg_dir, pcu, pixie_preprocessing):
    """Notebook 2, cells 20 -> 22 -> 26 with the given modules: smooth chanX (smooth_vals = 6), drop chanY's nuclear
    signal, then create_pixel_matrix over chan0, chan1, chanX_smoothed and chanY_nuc_exclude."""
    pcu.smooth_channels(COHORT_FOVS, tiff_dir, "TIFs", ["chanX"], 6)
    pcu.filter_with_nuclear_mask(COHORT_FOVS, tiff_dir, seg_dir, "chanY", img_sub_folder="TIFs", exclude=True)
    channels = ["chan0", "chan1", "chanX_smoothed", "chanY_nuc_exclude"]
    pixie_preprocessing.create_pixel_matrix(list(COHORT_FOVS), channels, td, tiff_dir, seg_dir,
                                            img_sub_folder="TIFs", subset_proportion=0.25, seed=42)
    return channels


def cohort_outputs(td, channels, read_dataframe):
    """What cells 20 -> 22 -> 26 leave behind, as arrays: the edited channel images, the three normalisation files and
    every FOV's full and sub-sampled table."""
    out = {}
    for fov in COHORT_FOVS:
        for ch in ("chanX_smoothed", "chanY_nuc_exclude"):
            out[f"edited_{fov}_{ch}"] = read_shaped(os.path.join(td, "tiffs", fov, "TIFs", ch + ".tiff"))
    for name, rel in (("pre", "pixel_output_dir/channel_norm_pre_rownorm.feather"),
                      ("thresh", "pixel_output_dir/pixel_thresh.feather"),
                      ("post", "channel_norm_post_rownorm.feather")):
        t = read_dataframe(os.path.join(td, rel))
        out[name + "_columns"] = np.array(list(t.columns), dtype="U24")
        out[name + "_values"] = t.values[0]
    for fov in COHORT_FOVS:
        for kind in ("pixel_mat_data", "pixel_mat_subsetted"):
            t = read_dataframe(os.path.join(td, kind, fov + ".feather"))
            tag = f"{kind}_{fov}"
            out[tag + "_columns"] = np.array(list(t.columns), dtype="U24")
            out[tag + "_dtypes"] = np.array([str(d) for d in t.dtypes], dtype="U16")
            out[tag + "_channels"] = t[channels].values
            out[tag + "_meta"] = t[["row_index", "column_index", "label"]].values.astype(np.int64)
    return out


POST_ULPS = 4


def check_cohort(got, want, same):
    """``got`` (cohort_outputs) against g16_cohort with ``same`` (dtype, shape and values), except the cohort's 99.9 %
    values (``post_values``), held to POST_ULPS ulp: they have differed by 1-2 ulp between runs, both between runs of
    the reference's own create_pixel_matrix (two regenerations of g16_cohort) and between CPU runs here, now and then
    and on the same inputs.  The cause is not established."""
    assert sorted(got) == sorted(k for k in want.files if k != "stdout")
    for k, v in got.items():
        if k == "post_values":
            assert v.dtype == want[k].dtype and v.shape == want[k].shape
            np.testing.assert_array_max_ulp(v, want[k], POST_ULPS)
        else:
            same(v, want[k])
