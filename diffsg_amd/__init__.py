"""diffsg_amd -- MI355X-native (gfx950) implementation of DiffSG's classifier-free DDPM hot path.

Host-side mirror of the reference's Python object API (ddpm_opt/*.py) over the C ABI of libdiffsg_hip.so
(include/diffsg.h).  See DESIGN.md.
"""
from .UNetCF import UNet1D  # noqa: F401
from .diffusion import generate_cosine_schedule, init_weights  # noqa: F401
from .ema import ExponentialMovingAverage  # noqa: F401
from .repeated import BestOf, best_of  # noqa: F401
from .mtfnn import MTFNN, co_net, msr_net  # noqa: F401
from .ppo import PPOAgent  # noqa: F401
from .steps import StepPlan, strided, ddim, tail  # noqa: F401
from .gd import co_descent, msr_descent, nu_descent, gd_co, gd_msr, gd_nu  # noqa: F401

__all__ = ["UNet1D", "generate_cosine_schedule", "init_weights", "ExponentialMovingAverage", "BestOf", "best_of", "MTFNN", "co_net", "msr_net",
           "PPOAgent", "StepPlan", "strided", "ddim", "tail", "co_descent", "msr_descent", "nu_descent", "gd_co", "gd_msr",
           "gd_nu"]
