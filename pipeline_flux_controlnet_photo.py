"""Module name in the style of the reference's two pipeline modules (`from pipeline_flux_controlnet_photo import
FluxControlNetPhotoPipeline`): the repaint call on a full-size photo — crop, resample and composite on the device — which the
reference does not have."""
from reptext_amd.pipeline import FluxPipelineOutput, calculate_shift, retrieve_latents, retrieve_timesteps  # noqa: F401
from reptext_amd.pipeline_photo import FluxControlNetPhotoPipeline, min_padding_for_blur, photo_crop_region  # noqa: F401
from reptext_amd.pipeline_repaint import repaint_t_start  # noqa: F401

__all__ = ["FluxControlNetPhotoPipeline", "FluxPipelineOutput", "calculate_shift", "min_padding_for_blur", "photo_crop_region", "repaint_t_start",
           "retrieve_latents", "retrieve_timesteps"]
