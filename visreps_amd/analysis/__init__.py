"""Mirror of visreps.analysis: rsa (RDM / RDM comparison / RSA) and alignment; beyond the
reference, neighbors (exact k-NN: nearest_k, mle_id, mutual_knn, mutual_knn_test,
compute_mutual_knn). Every module lists its public names in __all__."""
