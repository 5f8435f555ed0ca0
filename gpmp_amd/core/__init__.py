"""gpmp_amd.core -- GP model facade and its numerical routines (gpmp/core counterpart)."""
from .fourier_paths import PosteriorPaths, PriorPaths
from .model import Model
from .posterior_mean import PosteriorMean, PosteriorMeans

__all__ = ["Model", "PosteriorMean", "PosteriorMeans", "PosteriorPaths", "PriorPaths"]
