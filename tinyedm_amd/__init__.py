"""tinyedm_amd -- MI355X-native EDM/EDM2 training + sampling hot path: hand-written HIP kernels
(tinyedm_amd/csrc, C-ABI in include/tinyedm_hip.h) behind the tinyedm Python API.  The ``tinyedm``
alias package re-exports these names so reference configs (``_target_: tinyedm.EDM``) resolve."""
__version__ = "0.1.0"

from . import _runtime_env  # noqa: F401  (first: sets HIP runtime flags before anything can initialise the GPU)
from .cluster import KMeans, mode_report
from .compare import PairedQuality
from .edm import EDM, Diffuser
from .ema import EMA, EMAOptimizer, FusedAdam, sigma_rel_to_gamma
from .features import FeatureExtractor
from .frechet import DistributionDistance, FeatureStats, frechet_distance, kid, kid_from_sums, subset_indices
from .ideal import IdealDenoiser
from .metric import WeightedMeanSquaredError
from .networks import Conv2d, Denoiser, DenoiserWrapper, Embedding, Linear, manual_seed
from .prdc import ManifoldMetrics
from .schedule import Schedule, optimize_schedule
from .solvers import (AdaptiveSolver, DeterministicSolver, GaussianBlur, LinearDegradation, MultistepSolver,
                      ParallelSolver, ParallelStats, StochasticSolver, Trajectory)
from .trainer import LightningModule, Trainer
from .vjp import input_vjp
from . import cluster, config, networks, ops

__all__ = ["EDM", "Diffuser", "DeterministicSolver", "StochasticSolver", "MultistepSolver", "AdaptiveSolver", "ParallelSolver", "ParallelStats", "Trajectory", "Schedule", "optimize_schedule", "LinearDegradation", "GaussianBlur", "input_vjp", "IdealDenoiser", "FeatureExtractor", "PairedQuality", "ManifoldMetrics", "KMeans", "mode_report", "DistributionDistance", "FeatureStats", "frechet_distance", "kid", "kid_from_sums",
           "subset_indices", "WeightedMeanSquaredError", "Denoiser", "Linear", "Conv2d",
           "Embedding", "DenoiserWrapper", "EMA", "EMAOptimizer", "FusedAdam", "Trainer", "LightningModule",
           "sigma_rel_to_gamma", "manual_seed", "cluster", "config", "networks", "ops"]
