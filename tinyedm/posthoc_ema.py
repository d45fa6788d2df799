"""`python -m tinyedm.posthoc_ema ...` and `_target_: tinyedm.posthoc_ema.PostHocEMA`: the implementation lives in
tinyedm_amd.posthoc_ema."""
from tinyedm_amd.posthoc_ema import (PostHocEMA, build_parser, main, reconstruct, solve_coefficients,  # noqa: F401
                                     write_outputs)

if __name__ == "__main__":
    main()
