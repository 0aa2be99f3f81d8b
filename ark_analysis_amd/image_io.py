"""Single-channel TIFF images on disk, laid out the way the Pixie notebooks expect them:
``<tiff_dir>/<fov>/[<img_sub_folder>/]<channel>.tiff``.  The reference reads them through
``alpineer.load_utils.load_imgs_from_tree`` (scikit-image underneath); neither package is in this image, so
the few things the pixel path needs are done with Pillow: list a FOV's channels, read one channel, read a
stack of channels as ``[H, W, C]`` in the files' own dtype (float32 for MIBI/MPLEX exports)."""
import os
from typing import List, Optional, Sequence

import numpy as np

from .host_utils import natsorted

_EXTENSIONS = (".tiff", ".tif")


def _fov_folder(tiff_dir, fov: str, img_sub_folder: Optional[str]) -> str:
    return os.path.join(tiff_dir, fov, img_sub_folder or "")


def channel_names(tiff_dir, fov: str, img_sub_folder: Optional[str] = None) -> List[str]:
    """Channel names (file names without extension) present for ``fov``, naturally sorted."""
    folder = _fov_folder(tiff_dir, fov, img_sub_folder)
    return natsorted(os.path.splitext(f)[0] for f in os.listdir(folder)
                     if f.lower().endswith(_EXTENSIONS) and not f.startswith("."))


def _channel_file(folder: str, channel: str) -> str:
    for ext in _EXTENSIONS:
        path = os.path.join(folder, channel + ext)
        if os.path.exists(path):
            return path
    raise FileNotFoundError("The file/path, %s.tiff, could not be found in %s" % (channel, folder))


# Uncompressed TIFF strips are read straight from the file into the destination array (``readinto``: one copy, no
# GIL while the kernel copies), not through Pillow's decoder: ``np.array(im)`` runs Pillow's raw codec chunk by
# chunk from Python, ~1.2 GB/s per image and mostly under the GIL -- 16 decoder threads then starve the thread
# that drives the GPU (measured: the per-FOV percentile call, 4 ms alone, took 150 ms beside them).
# rawmode -> (dtype in the file, dtype Pillow's array would have)
_RAW_MODES = {"F;32F": ("<f4", np.float32), "F;32BF": (">f4", np.float32), "I;32S": ("<i4", np.int32),
              "I;32BS": (">i4", np.int32), "I;16": ("<u2", np.uint16), "I;16B": (">u2", np.uint16),
              "I;16S": ("<i2", np.int16), "I;16BS": (">i2", np.int16), "L": ("u1", np.uint8)}
# (signed 16-bit stays int16, as the tifffile-based reader of the reference returns it -- cluster masks are saved
# that way; Pillow's own decoder would widen it to int32)


def _raw_layout(im):
    """``(file dtype, array dtype, [(row0, row1, file offset), ...])`` when the opened image is a single page of
    uncompressed full-width strips in a sample format listed above; None otherwise (Pillow then decodes it)."""
    tiles = getattr(im, "tile", None)
    if not tiles or getattr(im, "n_frames", 1) != 1:
        return None
    width = im.size[0]
    mode, strips = None, []
    for tile in tiles:
        codec, extents, offset, args = tile[0], tile[1], tile[2], tile[3]
        if codec != "raw" or not isinstance(args, tuple) or len(args) < 3 or args[1] != 0 or args[2] != 1:
            return None
        if args[0] not in _RAW_MODES or (mode is not None and args[0] != mode):
            return None
        if extents[0] != 0 or extents[2] != width:
            return None
        mode = args[0]
        strips.append((extents[1], extents[3], offset))
    file_dtype, array_dtype = _RAW_MODES[mode]
    return np.dtype(file_dtype), np.dtype(array_dtype), strips


def _read_strips(path, shape, layout, out):
    """Fills ``out`` ([H, W], C-contiguous, dtype = layout's array dtype) from the file; False if the file is
    shorter than its directory says (the caller falls back to Pillow, which raises the proper error)."""
    file_dtype, array_dtype, strips = layout
    direct = file_dtype == array_dtype and file_dtype.isnative
    with open(path, "rb", buffering=0) as f:
        for row0, row1, offset in strips:
            rows = out[row0:row1]
            f.seek(offset)
            if direct:
                if f.readinto(memoryview(rows).cast("B")) != rows.nbytes:
                    return False
            else:
                block = np.fromfile(f, dtype=file_dtype, count=rows.size)
                if block.size != rows.size:
                    return False
                rows[...] = block.reshape(rows.shape)
    return True


def read_image(path, out=None) -> np.ndarray:
    """Any single image file as an array in its own dtype (what ``np.array(PIL.Image.open(path))`` returns).
    ``out``: a C-contiguous ``[H, W]`` array to fill when shape and dtype agree (else a new array is returned)."""
    from PIL import Image
    with Image.open(path) as im:
        layout = _raw_layout(im)
        if layout is not None:
            shape = (im.size[1], im.size[0])
            dest = out if (out is not None and out.shape == shape and out.dtype == layout[1]
                           and out.flags.c_contiguous) else np.empty(shape, dtype=layout[1])
            if _read_strips(path, shape, layout, dest):
                return dest
        return np.array(im)


# TIFF SampleFormat (1 unsigned, 2 signed, 3 float) and BitsPerSample -> numpy kind
_SAMPLE_KINDS = {1: "u", 2: "i", 3: "f"}


def _tiff_header(f, path):
    """``(byte order, offset of the first image directory)`` of an open TIFF; the offset is None for a BigTIFF."""
    import struct
    head = f.read(8)
    if len(head) < 8 or head[:2] not in (b"II", b"MM"):
        raise ValueError("%s is not a TIFF file" % path)
    bo = "<" if head[:2] == b"II" else ">"
    magic, first = struct.unpack(bo + "HI", head[2:8])
    return bo, (first if magic == 42 else None)


def _read_directory(f, bo, offset):
    """``({tag: values}, offset of the next directory or 0)`` of the image directory at ``offset`` of a classic TIFF."""
    import struct
    f.seek(offset)
    (count,) = struct.unpack(bo + "H", f.read(2))
    raw = f.read(12 * count + 4)
    sizes = {1: ("B", 1), 2: ("s", 1), 3: ("H", 2), 4: ("I", 4), 16: ("Q", 8)}
    tags = {}
    for i in range(count):
        tag, kind, n = struct.unpack(bo + "HHI", raw[12 * i:12 * i + 8])
        if kind not in sizes:
            continue
        code, size = sizes[kind]
        body = raw[12 * i + 8:12 * i + 12]
        if n * size > 4:
            (where,) = struct.unpack(bo + "I", body)
            f.seek(where)
            body = f.read(n * size)
        tags[tag] = body[:n] if code == "s" else struct.unpack(bo + code * n, body[:n * size])
    (next_ifd,) = struct.unpack(bo + "I", raw[12 * count:12 * count + 4])
    return tags, next_ifd


def _tiff_directory(path):
    """``(byte order, {tag: values})`` of the first image directory of a classic TIFF, plus whether more pages follow."""
    with open(path, "rb") as f:
        bo, first = _tiff_header(f, path)
        if first is None:
            return bo, None, False          # BigTIFF: left to Pillow
        tags, next_ifd = _read_directory(f, bo, first)
    return bo, tags, next_ifd != 0


def _shape_description(tags):
    """The array shape tifffile records in a page's ImageDescription (``{"shape": [...]}``), or None."""
    import json
    desc = tags.get(270)
    if not desc:
        return None
    try:
        meta = json.loads(bytes(desc).rstrip(b"\0").decode("ascii"))
        return tuple(int(d) for d in meta["shape"])
    except (ValueError, KeyError, TypeError, UnicodeDecodeError):
        return None


def read_tiff_shaped(path) -> np.ndarray:
    """A single-page TIFF as a tifffile-based reader (``skimage.io.imread``) returns it: in the file's own dtype (int64
    and the other 8-byte sample formats included) and in the shape its tifffile shape description records -- an array
    saved as ``(1, H, W)`` keeps its leading axis, where :func:`read_image` gives ``(H, W)``.  Without such a
    description the page's ``(H, W)``.  Uncompressed or deflate-compressed strips of one sample per pixel are read
    here; anything else goes through :func:`read_image`.  Multi-page files are not supported."""
    import zlib
    bo, tags, more = _tiff_directory(path)
    if more:
        raise NotImplementedError("%s: multi-page TIFF files are not supported" % path)
    arr = None
    if tags is not None:
        width, height = tags.get(256, (0,))[0], tags.get(257, (0,))[0]
        bits = tags.get(258, (1,))[0]
        kind = _SAMPLE_KINDS.get(tags.get(339, (1,))[0])
        compression, predictor = tags.get(259, (1,))[0], tags.get(317, (1,))[0]
        plain = (tags.get(277, (1,))[0] == 1 and 273 in tags and 279 in tags and kind is not None
                 and bits in (8, 16, 32, 64) and compression in (1, 8, 32946) and predictor in (1, 2)
                 and not (kind == "f" and (bits == 8 or predictor == 2)))
        if plain:
            dtype = np.dtype(bo + kind + str(bits // 8))
            chunks = []
            with open(path, "rb") as f:
                for offset, nbytes in zip(tags[273], tags[279]):
                    f.seek(offset)
                    data = f.read(nbytes)
                    chunks.append(zlib.decompress(data) if compression != 1 else data)
            flat = np.frombuffer(b"".join(chunks), dtype=dtype)
            if flat.size >= width * height:
                arr = flat[:width * height].reshape(height, width).astype(dtype.newbyteorder("="))
                if predictor == 2:          # horizontal differencing: running sums along each row, in the dtype
                    arr = np.cumsum(arr, axis=1, dtype=arr.dtype)
    if arr is None:
        arr = read_image(path)
    shape = _shape_description(tags or {})
    if shape is not None and int(np.prod(shape)) == arr.size:
        arr = arr.reshape(shape)
    return arr


def read_channel(tiff_dir, fov: str, channel: str, img_sub_folder: Optional[str] = None, out=None) -> np.ndarray:
    """One channel image ``[H, W]`` in the file's dtype."""
    return read_image(_channel_file(_fov_folder(tiff_dir, fov, img_sub_folder), channel), out=out)


_DECODERS = None


def _decoder_pool():
    """Shared thread pool for reading / decoding the channel files of a FOV side by side."""
    global _DECODERS
    if _DECODERS is None:
        from concurrent.futures import ThreadPoolExecutor
        _DECODERS = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4), thread_name_prefix="pxsom-tiff")
    return _DECODERS


def read_channels(tiff_dir, fov: str, channels: Sequence[str], img_sub_folder: Optional[str] = None) -> np.ndarray:
    """``[H, W, len(channels)]`` stack in the dtype of the first channel (the loader the reference uses
    allocates the stack with the dtype of a test image).  The channel files are decoded side by side into
    one channel-planar buffer and the result is that buffer VIEWED as ``[H, W, C]``: interleaving 22 planes
    on the host costs several times the decode, so it is left to the device (``flowsom`` uploads planar
    storage as it lies and permutes there); for numpy the view behaves like any other array."""
    channels = list(channels)
    first = read_channel(tiff_dir, fov, channels[0], img_sub_folder)
    planar = np.empty((len(channels),) + first.shape, dtype=first.dtype)
    planar[0] = first

    def fill(j):
        got = read_channel(tiff_dir, fov, channels[j], img_sub_folder, out=planar[j])
        if got is not planar[j]:       # another dtype / shape, or a compressed file: converted as numpy assigns
            planar[j] = got

    list(_decoder_pool().map(fill, range(1, len(channels))))
    return planar.transpose(1, 2, 0)


def iter_stacks(tiff_dir, fovs: Sequence[str], channels: Sequence[str], img_sub_folder: Optional[str] = None,
                cache: Optional[dict] = None, fill: bool = True):
    """Yields ``(fov, stack)`` for every FOV, reading one FOV ahead on a background thread.  ``cache``
    (fov -> stack) is consulted first and, with ``fill``, filled while it stays under
    ``cache['__max_bytes__']``: the passes create_pixel_matrix makes over the same TIFFs (two percentile passes, then the tables) decode them once
    when the cohort fits the budget."""
    from concurrent.futures import ThreadPoolExecutor
    fovs = list(fovs)

    def load(fov):
        if cache is not None and fov in cache:
            return cache[fov]
        stack = read_channels(tiff_dir, fov, channels, img_sub_folder)
        if cache is not None and fill:
            used = cache.get("__bytes__", 0)
            if used + stack.nbytes <= cache.get("__max_bytes__", 0):
                cache[fov] = stack
                cache["__bytes__"] = used + stack.nbytes
        return stack

    with ThreadPoolExecutor(max_workers=1, thread_name_prefix="pxsom-fov") as ahead:
        pending = ahead.submit(load, fovs[0]) if fovs else None
        for i, fov in enumerate(fovs):
            stack = pending.result()
            pending = ahead.submit(load, fovs[i + 1]) if i + 1 < len(fovs) else None
            yield fov, stack


def stack_cache(max_bytes: Optional[int] = None) -> dict:
    """A cache for :func:`iter_stacks`; default budget 8 GiB of host memory (``PXSOM_STACK_CACHE_GB``)."""
    if max_bytes is None:
        max_bytes = int(float(os.environ.get("PXSOM_STACK_CACHE_GB", "8")) * (1 << 30))
    return {"__max_bytes__": int(max_bytes), "__bytes__": 0}


def write_channel(path, image: np.ndarray) -> None:
    """Counterpart used by tests and the synthetic-cohort script."""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(image)).save(path, format="TIFF")


_SAMPLE_FORMATS = {"u": 1, "i": 2, "f": 3}


def write_image(path, image: np.ndarray) -> None:
    """A 2-D uint8 / uint16 / int16 / int32 / uint32 / float32 array as a baseline TIFF in its own dtype: little-endian,
    uncompressed, one strip, with the SampleFormat tag -- what the cluster masks are saved as (int16 stays int16,
    which Pillow cannot write).  :func:`read_image` reads it back unchanged (a uint32 file: :func:`read_tiff_shaped`)."""
    import struct
    image = np.asarray(image)
    if image.ndim != 2 or image.dtype.name not in ("uint8", "uint16", "int16", "int32", "uint32", "float32"):
        raise ValueError("write_image takes a 2-D uint8, uint16, int16, int32, uint32 or float32 array, got %s %s"
                         % (image.dtype, image.shape))
    data = np.ascontiguousarray(image, dtype=image.dtype.newbyteorder("<"))
    if data.nbytes >= 1 << 32:
        raise ValueError("image too large for a classic TIFF")
    height, width = data.shape
    short, long_ = 3, 4
    tags = [(256, long_, width), (257, long_, height), (258, short, data.dtype.itemsize * 8), (259, short, 1),
            (262, short, 1), (273, long_, 0), (277, short, 1), (278, long_, height), (279, long_, data.nbytes),
            (339, short, _SAMPLE_FORMATS[data.dtype.kind])]
    first_byte = 8 + 2 + 12 * len(tags) + 4
    directory = struct.pack("<H", len(tags))
    for tag, kind, value in tags:
        value = first_byte if tag == 273 else value
        directory += struct.pack("<HHI", tag, kind, 1) + (struct.pack("<HH", value, 0) if kind == short
                                                            else struct.pack("<I", value))
    with open(path, "wb") as f:
        f.write(b"II*\0" + struct.pack("<I", 8) + directory + struct.pack("<I", 0))
        f.write(memoryview(data).cast("B"))


# ---- multi-page stacks and colour images (K29: the Mesmer input, the overlays, the coloured masks) -------------------
_STACK_DTYPES = ("uint8", "uint16", "int16", "int32", "uint32", "float32")


def _directory_bytes(entries, offset, next_ifd):
    """An image directory placed at ``offset``: ``entries`` are ``(tag, kind, values)`` with kind 3 (SHORT) or 4 (LONG);
    values longer than four bytes lie right behind the directory."""
    import struct
    after = offset + 2 + 12 * len(entries) + 4
    body, extra = b"", b""
    for tag, kind, values in entries:
        raw = struct.pack("<%d%s" % (len(values), "H" if kind == 3 else "I"), *values)
        if len(raw) <= 4:
            field = raw.ljust(4, b"\0")
        else:
            field = struct.pack("<I", after + len(extra))
            extra += raw + (b"\0" if len(raw) % 2 else b"")
        body += struct.pack("<HHI", tag, kind, len(values)) + field
    return struct.pack("<H", len(entries)) + body + struct.pack("<I", next_ifd) + extra


def _page_entries(height, width, bits, sample_format, samples, strip_offset, nbytes):
    short, long_ = 3, 4
    entries = [(256, long_, (width,)), (257, long_, (height,)), (258, short, (bits,) * samples), (259, short, (1,)),
               (262, short, (2 if samples >= 3 else 1,)), (273, long_, (strip_offset,)), (277, short, (samples,)),
               (278, long_, (height,)), (279, long_, (nbytes,))]
    if samples == 4:
        entries.append((338, short, (2,)))          # ExtraSamples: unassociated alpha
    entries.append((339, short, (sample_format,) * samples))
    return entries


def _write_pages(path, pages, samples):
    """``pages``: C-contiguous little-endian arrays of one shape and dtype, each written as directory, then its one strip."""
    dtype = pages[0].dtype
    height, width = pages[0].shape[:2]
    bits, fmt = dtype.itemsize * 8, _SAMPLE_FORMATS[dtype.kind]
    nbytes = pages[0].nbytes
    dir_len = len(_directory_bytes(_page_entries(height, width, bits, fmt, samples, 0, nbytes), 0, 0))
    stride = dir_len + nbytes + (nbytes % 2)        # directories start on even offsets
    if 8 + stride * len(pages) >= 1 << 32:
        raise ValueError("image too large for a classic TIFF")
    with open(path, "wb") as f:
        f.write(b"II*\0\x08\0\0\0")
        for i, page in enumerate(pages):
            offset = 8 + i * stride
            entries = _page_entries(height, width, bits, fmt, samples, offset + dir_len, nbytes)
            f.write(_directory_bytes(entries, offset, offset + stride if i + 1 < len(pages) else 0))
            f.write(memoryview(page).cast("B"))
            if nbytes % 2:
                f.write(b"\0")


def write_stack(path, pages: np.ndarray) -> None:
    """A ``[P, H, W]`` uint8 / uint16 / int16 / int32 / uint32 / float32 array as a classic multi-page TIFF: little-endian,
    uncompressed, one strip per page, every page of the one shape and dtype -- the channels-first file
    ``generate_deepcell_input`` hands to Mesmer.  :func:`read_stack` reads it back unchanged."""
    pages = np.asarray(pages)
    if pages.ndim != 3 or pages.shape[0] < 1 or pages.size == 0 or pages.dtype.name not in _STACK_DTYPES:
        raise ValueError("write_stack takes a non-empty [P, H, W] uint8, uint16, int16, int32, uint32 or float32 array, "
                         "got %s %s" % (pages.dtype, pages.shape))
    data = np.ascontiguousarray(pages, dtype=pages.dtype.newbyteorder("<"))
    _write_pages(path, [data[i] for i in range(data.shape[0])], 1)


def write_rgb(path, image: np.ndarray) -> None:
    """A uint8 ``[H, W, 3]`` (RGB) or ``[H, W, 4]`` (RGB and unassociated alpha) array as a baseline TIFF: uncompressed,
    one strip, samples interleaved -- what the overlays and the coloured masks are saved as."""
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] not in (3, 4) or image.dtype != np.uint8 or image.size == 0:
        raise ValueError("write_rgb takes a non-empty uint8 [H, W, 3] or [H, W, 4] array, got %s %s" % (image.dtype, image.shape))
    _write_pages(path, [np.ascontiguousarray(image)], image.shape[2])


def read_stack(path) -> np.ndarray:
    """Every page of a TIFF as ``[P, H, W]`` in the file's own dtype (a single-page file gives ``P = 1``).  Uncompressed
    pages of one sample per pixel are read here strip by strip; a file holding anything else goes through Pillow page by
    page.  The pages must have one shape and dtype."""
    pages = None
    with open(path, "rb") as f:
        bo, offset = _tiff_header(f, path)
        if offset is not None:
            pages = []
            seen = set()
            while offset and pages is not None:
                if offset in seen:
                    raise ValueError("%s: its image directories form a loop" % path)
                seen.add(offset)
                tags, offset = _read_directory(f, bo, offset)
                width, height = tags.get(256, (0,))[0], tags.get(257, (0,))[0]
                bits = tags.get(258, (1,))[0]
                kind = _SAMPLE_KINDS.get(tags.get(339, (1,))[0])
                plain = (tags.get(277, (1,))[0] == 1 and 273 in tags and 279 in tags and kind is not None
                         and bits in (8, 16, 32, 64) and tags.get(259, (1,))[0] == 1 and not (kind == "f" and bits == 8)
                         and width > 0 and height > 0)
                if not plain:
                    pages = None
                    break
                chunks = []
                for where, nbytes in zip(tags[273], tags[279]):
                    f.seek(where)
                    chunks.append(f.read(nbytes))
                dtype = np.dtype(bo + kind + str(bits // 8))
                flat = np.frombuffer(b"".join(chunks), dtype=dtype)
                if flat.size < width * height:
                    pages = None
                    break
                pages.append(flat[:width * height].reshape(height, width).astype(dtype.newbyteorder("=")))
    if pages is None:
        from PIL import Image
        with Image.open(path) as im:
            pages = []
            for i in range(getattr(im, "n_frames", 1)):
                im.seek(i)
                pages.append(np.array(im))
    if any(p.shape != pages[0].shape or p.dtype != pages[0].dtype for p in pages):
        raise ValueError("%s: its pages differ in shape or dtype" % path)
    return np.stack(pages, axis=0)
