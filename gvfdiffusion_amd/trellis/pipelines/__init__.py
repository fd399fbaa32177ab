from .samplers import (FlowEulerSampler, FlowEulerCfgSampler, FlowEulerGuidanceIntervalSampler, sample_slat,  # noqa: F401
                       sample_sparse_structure, tokens_to_gaussians)
