"""gpmp_amd.core -- GP model facade and its numerical routines (gpmp/core counterpart)."""
from .model import Model
from .posterior_mean import PosteriorMean

__all__ = ["Model", "PosteriorMean"]
