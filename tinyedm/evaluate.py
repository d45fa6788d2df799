"""`python -m tinyedm.evaluate ...`: the implementation lives in tinyedm_amd.evaluate."""
from tinyedm_amd.evaluate import (NoiseLevelEvaluator, best_checkpoint, build_parser, check_args,  # noqa: F401
                                  check_sigmas, edm_weight, level_sigmas, level_stats, level_sums, main,
                                  merge_level_sums, report_entry)

if __name__ == "__main__":
    main()
