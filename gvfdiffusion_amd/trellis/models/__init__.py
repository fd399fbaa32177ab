from .structured_latent_vae import SLatGaussianDecoder, SparseTransformerBase  # noqa: F401
from .structured_latent_flow import SparseResBlock3d, ModulatedSparseTransformerCrossBlock, SLatFlowModel  # noqa: F401
