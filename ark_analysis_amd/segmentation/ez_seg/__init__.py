"""Mirror of the reference's ``ark.segmentation.ez_seg``: ``ez_object_segmentation`` (blur, threshold, hole filling,
connected-component labelling and the area filter on the device), ``merge_masks`` (object masks merged into the cell
segmentation: relabelling, overlap counts and the write pass on the device), ``composites`` (composite channels, host
numpy) and ``ez_seg_utils`` (the log writer, ``renumber_masks``)."""
