"""`python -m tinyedm.frechet ...`: the implementation lives in tinyedm_amd.frechet."""
from tinyedm_amd.frechet import (DistributionDistance, FeatureStats, build_parser, check_args, check_sets,  # noqa: F401
                                 feature_stats, format_table, frechet_distance, kid, kid_from_sums, main, subset_indices)

if __name__ == "__main__":
    main()
