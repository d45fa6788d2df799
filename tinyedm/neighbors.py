"""`python -m tinyedm.neighbors ...`: the implementation lives in tinyedm_amd.neighbors."""
from tinyedm_amd.neighbors import (NearestNeighbors, build_parser, check_args, closer_than_holdout,  # noqa: F401
                                   duplicates, load_images_u8, main, neighbour_rows, rms, summarize, write_grid)

if __name__ == "__main__":
    main()
