"""`python -m tinyedm.compare ...`: the implementation lives in tinyedm_amd.compare."""
from tinyedm_amd.compare import (PairedQuality, build_parser, check_args, gaussian_window, main, psnr_from_sse,  # noqa: F401
                                 read_pairs, region_from_box, run, uniform_window)

if __name__ == "__main__":
    main()
