"""The TRELLIS components next to the hot path: the structured-latent flow model and its Euler samplers
(trellis/models/structured_latent_flow.py, trellis/pipelines/samplers/), which turn sparse-structure coordinates and image-condition
tokens into the structured latent, and the structured-latent Gaussian decoder (trellis/models/structured_latent_vae/decoder_gs.py), whose
output is the canonical Gaussian set every frame of the path deforms.  The DINOv2 encoder, the dense sparse-structure flow stage and the
mesh / radiance-field decoders are out of scope."""
