"""Module name in the style of the reference's two pipeline modules (`from pipeline_flux_controlnet_repaint import
FluxControlNetRepaintPipeline`): latent-blend repaint of an existing image, which the reference does not have."""
from reptext_amd.pipeline import FluxPipelineOutput, calculate_shift, retrieve_latents, retrieve_timesteps  # noqa: F401
from reptext_amd.pipeline_repaint import FluxControlNetRepaintPipeline, repaint_t_start  # noqa: F401

__all__ = ["FluxControlNetRepaintPipeline", "FluxPipelineOutput", "calculate_shift", "repaint_t_start", "retrieve_latents", "retrieve_timesteps"]
