from .samplers import FlowEulerSampler, FlowEulerCfgSampler, FlowEulerGuidanceIntervalSampler, sample_slat  # noqa: F401
