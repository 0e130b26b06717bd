from . import diffusion, rectified_flow, transformer_diffusion  # noqa: F401
from .transformer_diffusion import ContinuousDiffusionOsuFusionDiT, DiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT  # noqa: F401
