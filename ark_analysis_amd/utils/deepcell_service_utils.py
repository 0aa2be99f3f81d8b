"""``ark.utils.deepcell_service_utils`` (the reference's ark/utils/deepcell_service_utils.py): ``generate_deepcell_input``,
the step that writes what Mesmer reads.  The rest of that module -- the request to the DeepCell service and its zip
helpers -- is network code and is not mirrored.

Each output is ``<data_dir>/<fov>.tiff`` with two pages, the sum of the nuclear channels and the sum of the membrane
channels, in the images' own dtype: ``np.sum(stack[..., chans], axis=2)`` assigned into that dtype.  On the device
 an integer stack is summed in 64 bits and narrowed, which is exactly numpy's sum and its wrapping
assignment; a float32 stack goes through pxsom_scaled_rowsum_f32 with a unit divisor, which adds a contiguous last axis
of up to 128 elements in numpy's order (``x / 1.0f`` is exact).  The stack is taken as C-contiguous ``[H, W, C]``: from 8
channels on numpy's order depends on the memory layout, and the layout alpineer and xarray hand to ``np.sum`` is
unpinned here (neither package is available)."""
import os

import numpy as np

from .. import image_io

_DEVICE_INT_DTYPES = ("uint8", "int16", "uint16", "int32", "uint32")
_MAX_FLOAT_CHANNELS = 128          # pxsom_scaled_rowsum_f32


# ---- device entry point (the CPU tests swap it for the numpy statement of the same contract) ------------------------
def _channel_sums_device(planar, groups):
    """``planar`` ``[C, H, W]`` (one of the device dtypes), ``groups`` lists of channel positions -> one ``[H, W]`` page
    per group in the stack's dtype."""
    import torch
    from .. import _capi, som_device
    dev = _capi.require_gpu()
    planar = np.ascontiguousarray(planar)
    c, h, w = planar.shape
    dtype = planar.dtype
    if dtype == np.float32:
        stack = torch.from_numpy(planar).to(dev).permute(1, 2, 0).reshape(h * w, c)
        pages = []
        for idx in groups:
            cols = stack[:, list(idx)].contiguous()
            ones = torch.ones(len(idx), dtype=torch.float32, device=dev)
            pages.append(som_device.scaled_rowsum_f32(cols, ones).reshape(h, w).cpu().numpy())
        return pages
    bits = dtype.itemsize * 8
    signed = np.dtype("int%d" % bits)
    wide = torch.from_numpy(planar.view(signed)).to(dev).to(torch.int64)
    if dtype.kind == "u":
        wide = wide & ((1 << bits) - 1)
    pages = []
    for idx in groups:
        total = wide[list(idx)].sum(dim=0)
        half = 1 << (bits - 1)
        narrowed = ((total + half) & ((1 << bits) - 1)) - half          # two's-complement wrap into `bits`
        pages.append(narrowed.to(getattr(torch, signed.name)).cpu().numpy().view(dtype))
    return pages


def _channel_sums_host(planar, groups):
    stack = np.ascontiguousarray(np.moveaxis(planar, 0, -1))
    pages = []
    for idx in groups:
        page = np.zeros(stack.shape[:2], dtype=stack.dtype)
        page[...] = np.sum(np.ascontiguousarray(stack[:, :, list(idx)]), axis=2)
        pages.append(page)
    return pages


def generate_deepcell_input(data_dir, tiff_dir, nuc_channels, mem_channels, fovs, is_mibitiff=False, img_sub_folder="TIFs",
                            dtype="int16"):
    """Saves the summed nuclear and membrane channels of every FOV of ``fovs`` (folders of ``tiff_dir``) as the two pages
    (nuclear, then membrane) of ``<data_dir>/<fov>.tiff``, in the images' own dtype; a page is zero when its channel list
    is empty.  ``dtype`` is accepted and unused, as in the reference's body.

    Raises ValueError when both channel lists are empty, NotImplementedError for ``is_mibitiff`` and for more than 128
    float32 channels in one sum."""
    if not nuc_channels and not mem_channels:
        raise ValueError("Either nuc_channels or mem_channels should be non-empty.")
    if is_mibitiff:
        raise NotImplementedError("MIBItiff input is not supported: save the channels as single-channel TIFFs")
    nuc = [c for c in (nuc_channels if nuc_channels else []) if c is not None]
    mem = [c for c in (mem_channels if mem_channels else []) if c is not None]
    channels = nuc + mem
    groups = [g for g in (list(range(len(nuc))), list(range(len(nuc), len(channels)))) if g]
    for fov in fovs:
        stack = image_io.read_channels(tiff_dir, fov, channels, img_sub_folder)        # [H, W, C], a view of [C, H, W]
        planar = np.moveaxis(stack, -1, 0)
        if planar.dtype == np.float32 and max(len(g) for g in groups) > _MAX_FLOAT_CHANNELS:
            raise NotImplementedError("generate_deepcell_input: more than %d float32 channels in one sum" % _MAX_FLOAT_CHANNELS)
        on_device = planar.dtype == np.float32 or planar.dtype.name in _DEVICE_INT_DTYPES
        pages = (_channel_sums_device if on_device else _channel_sums_host)(planar, groups)
        out = np.zeros((2,) + planar.shape[1:], dtype=planar.dtype)
        if nuc:
            out[0] = pages[0]
        if mem:
            out[1] = pages[-1]
        if out.dtype.name not in ("uint8", "uint16", "int16", "int32", "uint32", "float32"):
            raise NotImplementedError("generate_deepcell_input: %s images cannot be written as a TIFF stack" % out.dtype)
        image_io.write_stack(os.path.join(data_dir, f"{fov}.tiff"), out)
