"""Mirror of the reference's ``ark.segmentation.ez_seg`` for mask making: ``ez_object_segmentation`` (blur, threshold,
hole filling, connected-component labelling and the area filter on the device) and the log writer it uses."""
