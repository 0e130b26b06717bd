from . import attention, lora_layers, residual, scheduler, unet, utils  # noqa: F401
from .scheduler import GaussianDiffusionContinuousTimes  # noqa: F401
