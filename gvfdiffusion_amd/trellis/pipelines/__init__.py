from .samplers import (FlowEulerSampler, FlowEulerCfgSampler, FlowEulerGuidanceIntervalSampler, sample_slat,  # noqa: F401
                       sample_sparse_structure, tokens_to_gaussians)
from .image_encoder import encode_image, get_cond, image_to_gaussians, preprocess_image  # noqa: F401
