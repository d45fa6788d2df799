"""`python -m tinyedm.features ...`: the implementation lives in tinyedm_amd.features."""
from tinyedm_amd.features import (FeatureExtractor, RidgeProbe, best_cell, build_parser, check_args, format_table,  # noqa: F401
                                  knn_accuracy, knn_predict, knn_vote, main, ridge_probe, ridge_solve, write_features)

if __name__ == "__main__":
    main()
