"""`python -m tinyedm.schedule ...`: the implementation lives in tinyedm_amd.schedule."""
from tinyedm_amd.schedule import (Schedule, best_path, build_parser, format_schedule, load_schedules, main,  # noqa: F401
                                  optimize_schedule, save_schedules, schedules_from_costs, step_costs)

if __name__ == "__main__":
    main()
