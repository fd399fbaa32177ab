"""The TRELLIS components next to the hot path, from the image-condition tokens on: the sparse-structure stage
(trellis/models/sparse_structure_flow.py, sparse_structure_vae.py: the dense flow model over the 16^3 latent, the convolutional decoder to
occupancy logits and the read-out of the occupied cells), the structured-latent flow model and the Euler samplers
(trellis/models/structured_latent_flow.py, trellis/pipelines/samplers/), which turn those coordinates and the tokens into the structured
latent, and the structured-latent Gaussian decoder (trellis/models/structured_latent_vae/decoder_gs.py), whose output is the canonical
Gaussian set every frame of the path deforms.  The DINOv2 encoder, the sparse-structure encoder and the mesh / radiance-field decoders are
out of scope."""
