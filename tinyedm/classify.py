"""`python -m tinyedm.classify ...`: the implementation lives in tinyedm_amd.classify."""
from tinyedm_amd.classify import (DiffusionClassifier, best_checkpoint, build_parser, check_args,  # noqa: F401
                                  class_scores, class_weights, classification_stats, confusion_matrix,
                                  level_predictions, main, merge_counts, predict, report_entry)

if __name__ == "__main__":
    main()
