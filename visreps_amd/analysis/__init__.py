"""Mirror of visreps.analysis: rsa (RDM / RDM comparison / RSA) and alignment; beyond the
reference, neighbors (exact k-NN: nearest_k, mle_id, mutual_knn, mutual_knn_test,
compute_mutual_knn) and class_statistics, the label-conditioned analyses of the reference's
experiment scripts (class_moments / ClassMoments, pool_features, fisher_discriminant_per_dim,
class_centroid_importance, compute_csi, compute_layer_csi, class_selectivity, variance_ratio,
hoyer_sparsity, fraction_active). Every module lists its public names in __all__."""
