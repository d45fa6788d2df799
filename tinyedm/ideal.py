"""`python -m tinyedm.ideal ...`: the implementation lives in tinyedm_amd.ideal."""
from tinyedm_amd.ideal import (IdealDenoiser, build_parser, check_args, check_set, check_sigma, gap_report,  # noqa: F401
                               gap_sums, log_density, main, reduce_gap)

if __name__ == "__main__":
    main()
