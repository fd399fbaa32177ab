from .structured_latent_vae import SLatGaussianDecoder, SparseTransformerBase  # noqa: F401
from .structured_latent_flow import SparseResBlock3d, ModulatedSparseTransformerCrossBlock, SLatFlowModel  # noqa: F401
from .sparse_structure_vae import ResBlock3d, UpsampleBlock3d, SparseStructureDecoder, SparseStructureEncoder  # noqa: F401
from .sparse_structure_flow import ModulatedTransformerCrossBlock, SparseStructureFlowModel  # noqa: F401
