"""`python -m tinyedm.prdc ...`: the implementation lives in tinyedm_amd.prdc."""
from tinyedm_amd.prdc import (ManifoldMetrics, build_parser, check_args, check_k, check_sets, format_table,  # noqa: F401
                              main, metrics_from_counts, per_class, radii_from_knn)

if __name__ == "__main__":
    main()
