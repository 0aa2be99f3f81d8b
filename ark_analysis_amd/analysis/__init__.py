"""Mirror of the reference's ``ark.analysis`` for the neighbourhood matrix and its k-means clusters
(``neighborhood_analysis.create_neighborhood_matrix`` / ``generate_cluster_matrix_results``), with the neighbour counts
on the device, straight from the centroids.  See INTEGRATION.md."""
