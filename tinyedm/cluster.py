"""`python -m tinyedm.cluster ...`: the implementation lives in tinyedm_amd.cluster."""
from tinyedm_amd.cluster import (KMeans, build_parser, check_args, format_table, kmeans_plus_plus, lloyd_step,  # noqa: F401
                                 main, mode_report, read_clusters)

if __name__ == "__main__":
    main()
