"""Mirror of the reference's ``ark.segmentation`` for what consumes a finished segmentation: the cell table
(``marker_quantification.generate_cell_table``), with the per-cell reduction on the device.  See INTEGRATION.md."""
