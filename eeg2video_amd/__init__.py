"""eeg2video_amd -- the EEG2Video generation hot path (Tune-A-Video denoising loop + SD VAE) on MI355X.

Layout (only what the path needs):

* ``csrc/``      hand-written gfx950 kernels + the C-ABI library ``lib/libeeg2video_hip.so``
* ``_lib`` / ``engine``   ctypes binding and the one-ctx-per-GPU wrapper
* ``unet`` / ``vae`` / ``scheduler`` / ``pipeline``   mirrors of the reference's interfaces
  (``UNet3DConditionModel.forward`` / ``.from_pretrained``, ``AutoencoderKL``, the six scheduler types the pipeline's
  constructor accepts, ``TuneAVideoPipeline.__call__`` / ``.from_pretrained``)
* ``text_encoder`` / ``pipeline_tuneavideo``   ``transformers``' ``CLIPTextModel`` on the library and the text-prompt twin of the pipeline
* ``semantic`` / ``util``   the steps either side of the path: Semantic Predictor, DDIM inversion, ``save_videos_grid``
* ``metrics``   the reference's scoring script on the device: per-frame SSIM / MSE (``ssim_score_only`` ...), the image N-way
  accuracy (``img_classify_metric``) over ``image_classifier``, ``transformers``' ``ViTForImageClassification`` on the library, and
  the video N-way accuracy (``video_classify_metric``) over ``video_classifier``, its ``VideoMAEForVideoClassification``, and the
  CLIP score (``clip_score``, ``clip_score_only``, ``n_way_scores``) over ``clip_vision``, its ``CLIPVisionModelWithProjection``
* ``seq2seq``   the reference's Seq2Seq latent model ``myTransformer`` on the library: EEG windows in, UNet latents out
* ``features``  the reference's ``DE_PSD`` features of raw EEG on the library (``DE_PSD``, batched ``de_psd``)
* ``glmnet``    the reference's GLMNet pair ``glfnet`` / ``glfnet_mlp`` on the library: raw EEG or DE features in, logits / labels out
* ``host_models``   GLMNet / Seq2Seq as plain host-side torch modules (BASELINE configs[4] driver: ``examples/run_sweep.py``)
* ``weights``    state-dict key scheme + counter-RNG synthetic weights
* ``dist``       sharding of clips over ranks and the all-gather of decoded frames

The compute path has no CPU fallback: without the built library or without a GPU it raises.
"""
from .weights import (TINY_CLIP_VISION, TINY_GLMNET, TINY_IMAGE, TINY_SEMANTIC, TINY_SEQ2SEQ, TINY_TEXT, TINY_UNET, TINY_VAE, TINY_VIDEO,  # noqa: F401
                      ClipVisionConfig, GLMNetConfig, ImageConfig, SemanticConfig, Seq2SeqConfig, TextConfig, UNetConfig, VAEConfig, VideoConfig)

__all__ = ["UNetConfig", "VAEConfig", "TINY_UNET", "TINY_VAE", "Engine", "UNet3DConditionModel", "AutoencoderKL", "CLIPTextModel", "TextConfig", "ViTForImageClassification", "ImageConfig", "VideoMAEForVideoClassification", "VideoConfig", "CLIPVisionModelWithProjection", "ClipVisionConfig",
           "myTransformer", "Seq2Seq", "Seq2SeqConfig", "glfnet", "glfnet_mlp", "GLMNetConfig", "DE_PSD", "de_psd",
           "DDIMScheduler", "PNDMScheduler", "LMSDiscreteScheduler", "EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler",
           "DPMSolverMultistepScheduler", "TuneAVideoPipeline", "build_pipeline", "save_videos_grid"]


def __getattr__(name):          # lazy: importing the package must not need torch.cuda or the .so
    if name == "Engine":
        from .engine import Engine
        return Engine
    if name == "UNet3DConditionModel":
        from .unet import UNet3DConditionModel
        return UNet3DConditionModel
    if name == "CLIPTextModel":
        from .text_encoder import CLIPTextModel
        return CLIPTextModel
    if name == "ViTForImageClassification":
        from .image_classifier import ViTForImageClassification
        return ViTForImageClassification
    if name == "VideoMAEForVideoClassification":
        from .video_classifier import VideoMAEForVideoClassification
        return VideoMAEForVideoClassification
    if name == "CLIPVisionModelWithProjection":
        from .clip_vision import CLIPVisionModelWithProjection
        return CLIPVisionModelWithProjection
    if name in ("myTransformer", "Seq2Seq"):
        from .seq2seq import myTransformer
        return myTransformer
    if name in ("glfnet", "glfnet_mlp"):
        from . import glmnet
        return getattr(glmnet, name)
    if name in ("DE_PSD", "de_psd"):
        from . import features
        return getattr(features, name)
    if name == "AutoencoderKL":
        from .vae import AutoencoderKL
        return AutoencoderKL
    if name in ("DDIMScheduler", "PNDMScheduler", "LMSDiscreteScheduler", "EulerDiscreteScheduler",
                "EulerAncestralDiscreteScheduler", "DPMSolverMultistepScheduler"):
        from . import scheduler
        return getattr(scheduler, name)
    if name == "save_videos_grid":
        from .util import save_videos_grid
        return save_videos_grid
    if name in ("TuneAVideoPipeline", "build_pipeline"):
        from . import pipeline
        return getattr(pipeline, name)
    raise AttributeError(name)
