"""DiffusionPipeline / FluxPipeline: the reference's public API re-hosted on MI355X.

Signatures, defaults, return values and error behaviour follow
python/src/diffusionkit/mlx/__init__.py:64-594 (DiffusionPipeline), :597-671 (FluxPipeline),
:674-719 (CFGDenoiser), :722-747 (LatentFormat), :750-788 (append_dims, to_d, sample_euler).
Text-to-image and img2img (``image_path=``, ``denoise=``: VAE encoder, posterior sample per seed, truncated schedule) run as in the
reference; the text encoders (CLIP / T5, diffusionkit_amd.text) are built from the checkpoints ``local_ckpt`` names, and without
them ``encode_text`` falls back to deterministic synthetic conditioning so that ``generate_image`` stays callable end to end.
Checkpoint download is not offered (no hub access).

Inpainting (``mask_path=``, keyword-only, no reference counterpart) is latent blending on top of img2img: the mask (255 = repaint,
0 = keep) becomes one weight per latent cell, every Euler step re-imposes the known region re-noised to the step's sigma inside the
step's own launch (dk_euler_cfg_step_masked), and ``generate_image`` pastes the kept pixels of the input back over the decoded image
(``composite=``).  Kept latent cells come out as the encoded image bit for bit, kept pixels as the input's bytes.

Samplers (``sampler=``, keyword-only, no reference counterpart): "euler" (default: the reference's loop, ``sample_euler``), "heun" and "ab2" run
``sample_steps`` over the rows of ``sampler.step_plan`` -- one launch of dk_lms_cfg_step (or its masked form) behind every model evaluation.
FlowEdit (``edit_source_text=``, ``edit_steps=``, ``edit_n_avg=``, ``edit_source_cfg=``, keyword-only, no reference counterpart): text-guided editing
of ``image_path`` with the plain checkpoint -- ``sample_flowedit``, one launch of dk_flowedit_step behind every model evaluation, the source and the
target of a draw as batch rows of one evaluation, the noise drawn in the launch.
The stochastic samplers "euler_a" (``sampler_eta=``) and "sde" are rows with one more term, cn xi: their launch is dk_noisy_cfg_step, which draws xi
inside the launch from a counter (Philox4x32-10 keyed by the image's own seed), so no noise is drawn on the host, uploaded or stored per step.

Guidance (``guidance=``, ``guidance_interval=`` and the mode parameters, keyword-only, no reference counterpart; models that run with CFG): "cfg"
(default: today's combine), "rescale" and "apg" replace the step launch of ``sample_steps`` by dk_guided_cfg_step, and an interval runs the evaluations
outside it on the prompt rows alone (``_set_rows``).  The definitions are ``sampler.guide_reference``'s.

Skip-layer guidance (``skip_layer_guidance=``, ``skip_layers=``, ``skip_layer_interval=``, keyword-only, no reference counterpart; the recipe published with
Stable Diffusion 3.5 medium): in the steps of its window the engine carries a third row group, a copy of the prompt rows that joins in front of the first
skipped block and sits out the skipped ones (``MMDiTEngine.set_skip_layers``), and the step launch is dk_slg_cfg_step, which adds scale (c - k) to the
mode's prediction.  The definition is ``sampler.slg_reference``'s.  Arithmetic only, on synthetic weights: no SD3.5-medium checkpoint has been run here.

Perturbed-attention guidance (``pag_scale=``, ``pag_layers=``, ``pag_interval=``, keyword-only, no reference counterpart; diffusers'
StableDiffusion3PAGPipeline): the same third row group and the same step launch, but the fork rows run every block, and in the named ones their image
queries attend to the text keys and to their own key only (``MMDiTEngine.set_perturbed_attention``, dk_attention_identity_*).  One loop serves both
features (``_Loop.forked``); they cannot be combined: the engine forks one row group.  Arithmetic only, on synthetic weights.

All arithmetic runs in libdk_hip.so on the current HIP stream; numpy is used exactly where the
reference uses it (the seeded noise draw, __init__.py:553-557) and for O(num_steps) schedule
scalars.
"""
from __future__ import annotations

import hashlib
import logging
import time
from dataclasses import replace
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .config import (MMDIT_CKPT, MODEL_CONFIG, SKIP_LAYER_GUIDANCE, T5_MAX_LENGTH, MMDiTConfig, VAEDecoderConfig, VAEEncoderConfig)
from .engine import MMDiTEngine, VAEDecoderEngine, VAEEncoderEngine, _stream
from .sampler import (STOCHASTIC_SAMPLERS, FluxSampler, ModelSamplingDiscreteFlow, check_guidance, check_interval, check_perturbed_attention_guidance,
                      check_sampler, check_sampler_eta, check_skip_layer_guidance, get_sigmas,
                      guidance_rows, max_denoise, slg_rows, step_plan)
from .weights import pack_mmdit, pack_vae, synth_mmdit_weights, synth_vae_encoder_weights, synth_vae_weights

logger = logging.getLogger(__name__)
Tensor = torch.Tensor


def _round_to_dtype(x: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dtype).to(torch.float32).numpy()


def bytes2gigabytes(n: int) -> float:
    """python/src/diffusionkit/utils.py:42-44"""
    return n / 1024 ** 3


class LatentFormat:
    """mlx/__init__.py:722-733"""

    def __init__(self):
        self.scale_factor = 1.0
        self.shift_factor = 0.0

    def process_in(self, latent: Tensor) -> Tensor:
        return _affine(latent, self.scale_factor, -self.shift_factor * self.scale_factor)

    def process_out(self, latent: Tensor) -> Tensor:
        return _affine(latent, 1.0 / self.scale_factor, self.shift_factor)


class SD3LatentFormat(LatentFormat):
    def __init__(self):
        super().__init__()
        self.scale_factor = 1.5305
        self.shift_factor = 0.0609


class FluxLatentFormat(LatentFormat):
    def __init__(self):
        super().__init__()
        self.scale_factor = 0.3611
        self.shift_factor = 0.1159


def _open_image(image):
    """a path, a PIL image or a uint8 array -> PIL image"""
    from PIL import Image
    if isinstance(image, np.ndarray):
        return Image.fromarray(image)
    if isinstance(image, Image.Image):
        return image
    return Image.open(image)


def read_image_u8(image_path) -> np.ndarray:
    """The pixels ``DiffusionPipeline.read_image`` settles on (mlx/__init__.py:536-551), as HWC uint8 RGB: sizes are cut down to a multiple
    of 64 with a LANCZOS resize.  ``image_path`` may also be a PIL image or an HWC uint8 array.  Needs no GPU."""
    from PIL import Image
    img = _open_image(image_path)
    W, H = (dim - dim % 64 for dim in (img.width, img.height))
    if W != img.width or H != img.height:
        logger.warning(f"Warning: image shape is not divisible by 64, downsampling to {W}x{H}")
        img = img.resize((W, H), Image.LANCZOS)
    arr = np.array(img)
    if arr.ndim == 2:
        arr = np.repeat(arr[:, :, None], 3, axis=2)
    return arr[:, :, :3]


def read_mask(mask, size) -> np.ndarray:
    """Inpainting mask -> uint8 [H, W] with ``size`` = (H, W), the size ``read_image`` settled on: 255 = repaint, 0 = keep, values between
    blend.  ``mask`` is a path, a PIL image or an array ([H, W] or [H, W, channels], uint8 or bool); only the first channel is taken, and a
    mask of another size is resized with NEAREST, so that a {0, 255} mask stays one.  Needs no GPU."""
    from PIL import Image
    if isinstance(mask, np.ndarray):
        arr = mask
    else:
        img = _open_image(mask)
        if img.mode not in ("L", "RGB", "RGBA", "1"):
            img = img.convert("L")
        arr = np.array(img)
    if arr.ndim == 3:
        arr = arr[:, :, 0]
    if arr.ndim != 2:
        raise ValueError(f"mask must be [H, W] or [H, W, channels], got shape {arr.shape}")
    if arr.dtype == np.bool_:
        arr = arr.astype(np.uint8) * 255
    if arr.dtype != np.uint8:
        raise ValueError(f"mask must be uint8 (255 = repaint, 0 = keep) or bool, got {arr.dtype}")
    H, W = int(size[0]), int(size[1])
    if arr.shape != (H, W):
        arr = np.array(Image.fromarray(np.ascontiguousarray(arr)).resize((W, H), Image.NEAREST))
    return np.ascontiguousarray(arr)


def _read_masks(mask, size, n_img: int) -> np.ndarray:
    """uint8 [1, H, W] (one mask for all images) or, for a list / tuple of ``n_img`` masks, [n_img, H, W]"""
    if isinstance(mask, (list, tuple)):
        if len(mask) != n_img:
            raise ValueError(f"{len(mask)} masks for {n_img} images: give one mask, or one per image")
        return np.stack([read_mask(m, size) for m in mask], 0)
    return read_mask(mask, size)[None]


def read_reference_u8(image) -> np.ndarray:
    """A reference image (``reference_image_path=``) as HWC uint8 RGB: a path, a PIL image or an array, as ``read_image_u8`` takes them, but
    never resized -- sides that are not multiples of 16 pixels (one 2 x 2 patch of 8-pixel latent cells) raise.  Needs no GPU."""
    arr = np.array(_open_image(image))
    if arr.ndim == 2:
        arr = np.repeat(arr[:, :, None], 3, axis=2)
    arr = arr[:, :, :3]
    H, W = arr.shape[:2]
    if H < 16 or W < 16 or H % 16 or W % 16:
        raise ValueError(f"the reference image is {H}x{W}: both sides must be multiples of 16 pixels (it is not resized here)")
    return np.ascontiguousarray(arr)


def _read_references(reference, n_img: int) -> np.ndarray:
    """uint8 [1, H, W, 3] (one reference for all images) or, for a list / tuple of ``n_img`` references of one size, [n_img, H, W, 3]"""
    if isinstance(reference, (list, tuple)):
        if len(reference) != n_img:
            raise ValueError(f"{len(reference)} reference images for {n_img} images: give one reference, or one per image")
        refs = [read_reference_u8(r) for r in reference]
        if any(r.shape != refs[0].shape for r in refs):
            raise ValueError("the reference images of one call must have one size: " + ", ".join(f"{r.shape[0]}x{r.shape[1]}" for r in refs))
        return np.stack(refs, 0)
    return read_reference_u8(reference)[None]


_REFERENCE_NEEDS_ROPE = ("reference_image_path needs a FLUX-family pipeline: the reference image's tokens are told from the image's by their RoPE "
                         "position index, and the SD3 family has no RoPE")


CONDITION_FEATURES = {"fill": 320, "control": 64}  # condition= of FluxPipeline -> MMDiTConfig.condition_features (FLUX_FILL_DEV / FLUX_CONTROL_DEV)


_CONDITION_NEEDS_FLUX = ("channel-concatenated conditioning (condition / condition_image_path / condition_mask_path) needs a FLUX-family pipeline: "
                         "FLUX.1 Fill / Canny / Depth are FLUX.1-dev checkpoints, and the SD3 family's x_embedder has no condition columns")


def check_condition_kind(kind, is_flux: bool) -> None:
    """``condition=`` of a pipeline's constructor: None, or "fill" / "control" on the FLUX family.  Needs no GPU."""
    if kind is None:
        return
    if not is_flux:
        raise ValueError(_CONDITION_NEEDS_FLUX)
    if kind not in CONDITION_FEATURES:
        raise ValueError(f"unknown condition {kind!r} (fill | control)")


def check_condition_args(kind, condition_image, condition_mask, reference, is_flux: bool) -> None:
    """The rules of channel-concatenated conditioning (``FluxPipeline(condition=)``, ``condition_image_path=`` / ``condition_mask_path=``), checked
    before any GPU work; ``kind`` is the pipeline's ``condition``.  Needs no GPU."""
    if kind is None and condition_image is None and condition_mask is None:
        return
    if not is_flux:
        raise ValueError(_CONDITION_NEEDS_FLUX)
    if kind is None:
        raise ValueError("condition_image_path / condition_mask_path need a pipeline built with condition='fill' or condition='control' "
                         "(its x_embedder weight carries the condition's columns)")
    check_condition_kind(kind, is_flux)
    if condition_image is None:
        raise ValueError(f"a pipeline built with condition={kind!r} needs condition_image_path in every call: the model was trained to see it")
    if kind == "fill" and condition_mask is None:
        raise ValueError("condition='fill' needs condition_mask_path: the mask says where to repaint (255) and what to keep (0)")
    if kind == "control" and condition_mask is not None:
        raise ValueError("condition='control' takes no condition_mask_path: the control image (edges, depth) conditions the whole picture")
    if reference is not None:
        raise ValueError("reference_image_path cannot be combined with condition_image_path: the engine carries one kind of image conditioning at a time")


def _mask_hw(mask):
    """(H, W) of a mask as ``read_mask`` takes it, without resizing anything"""
    if isinstance(mask, np.ndarray):
        return tuple(mask.shape[:2])
    img = _open_image(mask)
    return (img.height, img.width)


def read_condition_images(image, mask, size, n_img: int):
    """``condition_image_path`` / ``condition_mask_path`` -> (uint8 [1 or n_img, H, W, 3], uint8 [1 or n_img, H, W] or None): a path, a PIL image or an
    array each, or a list with one per image.  ``size`` = (H, W) of the output; nothing is resized, any other size raises.  Needs no GPU."""
    H, W = int(size[0]), int(size[1])

    def many(value, what):
        if isinstance(value, (list, tuple)):
            if len(value) != n_img:
                raise ValueError(f"{len(value)} condition {what}s for {n_img} images: give one, or one per image")
            return list(value)
        return [value]

    def one_image(v):
        arr = np.array(_open_image(v))
        if arr.ndim == 2:
            arr = np.repeat(arr[:, :, None], 3, axis=2)
        arr = arr[:, :, :3]
        if arr.dtype != np.uint8 or arr.shape != (H, W, 3):
            raise ValueError(f"the condition image is {arr.shape[0]}x{arr.shape[1]} ({arr.dtype}), the output {H}x{W}: it must be uint8 RGB of the "
                             "output's size (it is not resized here)")
        return np.ascontiguousarray(arr)

    def one_mask(v):
        if _mask_hw(v) != (H, W):
            raise ValueError(f"the condition mask is {_mask_hw(v)[0]}x{_mask_hw(v)[1]}, the output {H}x{W}: it must have the output's size (it is not "
                             "resized here)")
        return read_mask(v, (H, W))

    images = np.stack([one_image(v) for v in many(image, "image")], 0)
    masks = None if mask is None else np.stack([one_mask(v) for v in many(mask, "mask")], 0)
    return images, masks


def _affine(x: Tensor, a: float, b: float) -> Tensor:
    x = x.contiguous()
    y = torch.empty_like(x)
    lib = _lib.load()
    _lib.check(lib.dk_affine_f32(x.data_ptr(), y.data_ptr(), x.numel(), a, b, _stream()), "dk_affine_f32")
    return y


class DiffusionPipeline:
    _IS_FLUX = False

    def __init__(
        self,
        w16: bool = False,
        shift: float = 1.0,
        use_t5: bool = True,
        model_version: str = "argmaxinc/mlx-stable-diffusion-3-medium",
        low_memory_mode: bool = True,
        a16: bool = False,
        local_ckpt=None,
        *,
        device: Union[str, torch.device, None] = None,
        mmdit_config: Optional[MMDiTConfig] = None,
        vae_config: Optional[VAEDecoderConfig] = None,
        vae_encoder_config: Optional[VAEEncoderConfig] = None,
        weights_seed: int = 1234,
        text_len: Optional[int] = None,
        packed_weights: Optional[dict] = None,
        activation_dtype: Optional[str] = None,
        vae_dtype: Optional[str] = None,
        condition: Optional[str] = None,
        controlnet_ckpt=None,
        controlnet_config: Optional[MMDiTConfig] = None,
        ip_adapter_ckpt=None,
        ip_adapter_config=None,
    ):
        """``ip_adapter_ckpt`` (FluxPipeline only): a FLUX IP-Adapter in XLabs-AI's layout (flux-ip-adapter as diffusers'
        FluxIPAdapterJointAttnProcessor2_0 runs it) -- a .safetensors path or a state dict in that layout, or a dict of the names of
        ``weights.synth_ip_adapter_weights`` -- bound into the model's engine; ``ip_adapter_config``: a ``config.IPAdapterConfig`` (default
        ``config.FLUX_IP_ADAPTER``: 4 tokens of 4096 features from a 768-wide CLIP image embedding).  Every call must then name its
        ``ip_adapter_image_embeds`` (see ``denoise_latents``).  Refused on the SD3 family, on an fp8 engine, together with ``condition`` and with
        ``controlnet_ckpt`` (the LayerNorm launch has one tap operand).  The CLIP vision tower, several adapters at once, negative image embeds and
        InstantX's layout are not built.  Written from the published definition, arithmetic parity on synthetic weights only: no adapter
        checkpoint has been run, and nothing here says anything about image quality.
        ``controlnet_ckpt`` (SD3 family only): an SD3 ControlNet in the layout of diffusers' SD3ControlNetModel -- a .safetensors path or a state
        dict in that layout, or a dict of reference-named tensors (``weights.synth_mmdit_weights`` of a control-net config) -- built into a second
        ``MMDiTEngine``, ``self.controlnet``; ``controlnet_config``: its configuration (default ``config.SD3_CONTROLNET_6``, in the model's element
        type).  Every call must then name its ``controlnet_image_path`` (see ``denoise_latents``).  Refused on a model with dual attention
        blocks (SD3.5-medium) and on an fp8 engine.  On a ``FluxPipeline`` the ControlNet is a FLUX one in the layout of diffusers'
        FluxControlNetModel (double- and single-block taps) and ``controlnet_config`` is REQUIRED -- ``config.flux_controlnet_config(n_double,
        n_single)``: FLUX ControlNets have no canonical depth; refused there together with ``condition`` and an fp8 engine, and at the call with a
        reference image or ``block_cache``.  Arithmetic parity on synthetic weights only: no ControlNet checkpoint has been run.
        ``condition`` (FluxPipeline only): None, "fill" (FLUX.1 Fill) or "control" (FLUX.1 Canny / Depth) -- channel-concatenated conditioning: the
        model's x_embedder is 64 + 320 / 64 + 64 columns wide (``config.FLUX_FILL_DEV`` / ``FLUX_CONTROL_DEV``; a ``mmdit_config`` of the caller's
        gets that width), and every call must name its ``condition_image_path`` (see ``denoise_latents``).
        ``vae_dtype``: element type of the VAE decoder and (built on first use, img2img) encoder -- None or "bfloat16": bf16, today's
        behaviour bit for bit, also together with ``activation_dtype="float16"``; "float16": fp16 weights, activations and image tail.  It is the
        VAE's own switch and is accepted for every family: float16 is the reference's decoder dtype for Stable Diffusion 3
        (mlx/__init__.py:108-113,483-484), not for FLUX (bf16 there); the reference's encoder runs in fp32, so the fp16 encoder is the closer
        16-bit form, not its dtype.  ``packed_weights["vae_decoder"]`` / ``["vae_encoder"]`` must then hold float16 tensors (pack_vae with a
        float16_vae_config)."""
        check_condition_kind(condition, self._IS_FLUX)  # (before anything is loaded)
        self.condition = condition
        _lib.load()  # fail loudly before anything else if the HIP extension is missing
        # The MI355X build computes in bf16 end to end (BASELINE.json configs); w16/a16 are
        # accepted for signature compatibility.  The reference's defaults (w16 = a16 = False) mean fp32 weights / activations
        # there (mlx/__init__.py:76-79): say at run time that this build does not offer that mode instead of silently changing it
        if not (w16 and a16):
            logger.warning(f"w16={w16}, a16={a16}: fp32 weights / activations are not offered by the MI355X build; "
                           "computing with bf16 weights and bf16 activations (fp32 accumulation, fp32 latent state)")
        self.float16_dtype = torch.bfloat16
        self.dtype = torch.bfloat16
        self.activation_dtype = torch.bfloat16
        # activation_dtype="float16": the MMDiT engine, the conditioning hand-over, the CFG denoiser and the Euler loop run in the reference's
        # dtype for Stable Diffusion 3 (fp16 weights and activations, mlx/__init__.py:76-79); the text encoders stay bf16, the VAE has its own
        # switch, vae_dtype.  None (default): bf16, exactly as before
        if activation_dtype not in (None, "bfloat16", "float16"):
            raise ValueError(f"unknown activation_dtype {activation_dtype!r} (bfloat16 | float16)")
        if activation_dtype == "float16":
            if self._IS_FLUX:
                raise ValueError("activation_dtype float16 is the SD3 family's (head_dim 64, no single-stream blocks); FLUX runs in bfloat16")
            self.float16_dtype = self.dtype = self.activation_dtype = torch.float16
        # The model timesteps are host floats rounded to the REFERENCE pipeline's 16-bit dtype (quirk Q1): mx.float16 for
        # DiffusionPipeline (mlx/__init__.py:76-79,683,770), mx.bfloat16 for FluxPipeline (:610-613) -- 857.69 -> 857.5 in
        # fp16, 856 in bf16; the adaLN table is computed on these values.
        self.timestep_dtype = torch.bfloat16 if self._IS_FLUX else torch.float16
        self.use_t5 = use_t5
        self.mmdit_ckpt = MMDIT_CKPT[model_version]  # KeyError on unknown versions, as the reference
        self.low_memory_mode = low_memory_mode
        self.model_version = model_version
        self.local_ckpt = local_ckpt
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.mmdit_config = mmdit_config or MODEL_CONFIG[model_version]
        if condition is not None:
            from .config import FLUX_CONTROL_DEV, FLUX_FILL_DEV
            preset = FLUX_FILL_DEV if condition == "fill" else FLUX_CONTROL_DEV
            self.mmdit_config = preset if mmdit_config is None else replace(mmdit_config, condition_features=preset.condition_features)
        if activation_dtype is not None:
            from .config import validate_activation_dtype
            self.mmdit_config = replace(self.mmdit_config, activation_dtype=activation_dtype)
            validate_activation_dtype(self.mmdit_config)
        elif self.mmdit_config.activation_dtype == "float16":  # a float16_config() passed as mmdit_config
            self.float16_dtype = self.dtype = self.activation_dtype = torch.float16
        self.vae_config = vae_config or VAEDecoderConfig()
        self.vae_encoder_config = vae_encoder_config or VAEEncoderConfig()
        if vae_dtype is not None:
            from .config import float16_vae_config
            self.vae_config = float16_vae_config(self.vae_config, vae_dtype)  # (ValueError for an unknown name)
            self.vae_encoder_config = float16_vae_config(self.vae_encoder_config, vae_dtype)
        self.weights_seed = weights_seed
        self._text_len_override = text_len
        self._packed_weights = packed_weights  # {"mmdit": ..., "vae_decoder": ...} already in engine layout
        self._text_encoder: Optional[Callable] = None
        self._init_sampler(shift)
        self.ip_adapter_config, self._ip_adapter_named, self.last_ip_adapter = None, None, None
        if ip_adapter_ckpt is None and ip_adapter_config is not None:
            raise ValueError("ip_adapter_config needs ip_adapter_ckpt: there is no IP-Adapter to configure")
        if ip_adapter_ckpt is not None:
            _check_ip_adapter_config(self, ip_adapter_config, controlnet_ckpt)  # (before anything is loaded)
            from .model_io import load_ip_adapter_checkpoint
            self._ip_adapter_named = dict(load_ip_adapter_checkpoint(ip_adapter_ckpt, self.mmdit_config, self.ip_adapter_config))
        self.controlnet = None
        if controlnet_ckpt is None and controlnet_config is not None:
            raise ValueError("controlnet_config needs controlnet_ckpt: there is no ControlNet to configure")
        if controlnet_ckpt is not None:
            self._check_controlnet_config(controlnet_config)  # (before anything is loaded)
        self.check_and_load_models()
        if controlnet_ckpt is not None:
            self.load_controlnet(controlnet_ckpt)

    def _check_controlnet_config(self, controlnet_config) -> None:
        from .config import SD3_CONTROLNET_6, validate_control_net
        cfg = self.mmdit_config
        if self._IS_FLUX or cfg.depth_unified > 0:
            return _check_flux_controlnet_config(self, controlnet_config)
        if controlnet_config is not None and getattr(controlnet_config, "control_net_flux", False):
            raise ValueError("controlnet_config is a FLUX ControlNet's (control_net_flux=True): an SD3 pipeline takes an SD3 ControlNet (control_net=True)")
        if cfg.dual_attention_blocks > 0:
            raise ValueError("controlnet_ckpt cannot be combined with dual attention blocks (SD3.5-medium): the engine adds taps in a plain block's "
                             "LayerNorm launch only")
        if cfg.weight_dtype == "fp8_e4m3":
            raise ValueError("controlnet_ckpt cannot be combined with an fp8 engine: the taps are added on the bf16 / fp16 path only")
        ccfg = replace(controlnet_config or SD3_CONTROLNET_6, activation_dtype=cfg.activation_dtype)
        if not ccfg.control_net:
            raise ValueError("controlnet_config must be a control-net configuration (control_net=True, e.g. config.SD3_CONTROLNET_6)")
        validate_control_net(ccfg)
        if ccfg.hidden_size != cfg.hidden_size or ccfg.patch_dim != cfg.patch_dim or ccfg.depth_multimodal > cfg.depth_multimodal:
            raise ValueError(f"the ControlNet (hidden {ccfg.hidden_size}, patch_dim {ccfg.patch_dim}, {ccfg.depth_multimodal} blocks) does not fit the model "
                             f"(hidden {cfg.hidden_size}, patch_dim {cfg.patch_dim}, {cfg.depth_multimodal} blocks): the taps are added to its stream")
        self.controlnet_config = ccfg

    def load_controlnet(self, ckpt) -> None:
        """Builds ``self.controlnet``, the ControlNet's engine, from a path / state dict in the diffusers layout or reference-named tensors"""
        from .model_io import load_controlnet_checkpoint
        ccfg = self.controlnet_config
        named = dict(load_controlnet_checkpoint(ckpt, ccfg))
        self.controlnet = MMDiTEngine(ccfg, pack_mmdit(ccfg, named, self.device, consume=True))

    def _init_sampler(self, shift):
        self.sampler = ModelSamplingDiscreteFlow(shift=shift)
        self.latent_format = SD3LatentFormat()
        self.use_clip_g = True

    # -- model loading ---------------------------------------------------------------------
    def load_mmdit(self, only_modulation_dict: bool = False):
        """Builds the MMDiT engine.  ``local_ckpt`` may be a dict of reference-named tensors;
        otherwise seeded synthetic weights are used (no checkpoints exist in this environment)."""
        cfg = self.mmdit_config
        ipc = getattr(self, "ip_adapter_config", None)
        if ipc is not None:  # (the adapter's stacked K / V matrix and projection model ride in the model's dict: the engine binds them by name)
            return self._load_mmdit_with_adapter(cfg, ipc)
        if self._packed_weights is not None and "mmdit" in self._packed_weights:
            self.mmdit = MMDiTEngine(cfg, self._packed_weights["mmdit"])
            return
        if isinstance(self.local_ckpt, dict) and "mmdit" in self.local_ckpt:
            # a .safetensors path or a state dict, in BFL FLUX / Stability SD3 / reference key layout
            from .model_io import load_mmdit_checkpoint
            named = dict(load_mmdit_checkpoint(self.local_ckpt["mmdit"], cfg))
        else:
            named = synth_mmdit_weights(cfg, seed=self.weights_seed, device=self._synth_device(cfg.param_count()))
        self.mmdit = MMDiTEngine(cfg, pack_mmdit(cfg, named, self.device, consume=True))

    def _load_mmdit_with_adapter(self, cfg, ipc) -> None:
        """``load_mmdit`` for a pipeline built with ``ip_adapter_ckpt``: the same sources for the model's weights, the adapter's beside them"""
        from .weights import pack_ip_adapter
        if self._packed_weights is not None and "mmdit" in self._packed_weights:
            packed = dict(self._packed_weights["mmdit"])
        elif isinstance(self.local_ckpt, dict) and "mmdit" in self.local_ckpt:
            from .model_io import load_mmdit_checkpoint
            packed = pack_mmdit(cfg, dict(load_mmdit_checkpoint(self.local_ckpt["mmdit"], cfg)), self.device, consume=True)
        else:
            named = synth_mmdit_weights(cfg, seed=self.weights_seed, device=self._synth_device(cfg.param_count()))
            packed = pack_mmdit(cfg, named, self.device, consume=True)
        packed.update(pack_ip_adapter(cfg, ipc, self._ip_adapter_named, self.device))
        self.mmdit = MMDiTEngine(cfg, packed, ip_adapter=ipc)

    def _synth_device(self, n_params: int):
        """Seeded synthetic weights come from the CPU generator stream (the one the oracle and the
        parity tests draw from) unless the model is too large to draw on the host in reasonable time;
        above 1e9 parameters the device generator is used (a different, equally seeded stream)."""
        return "cpu" if n_params < 1_000_000_000 else self.device

    def check_and_load_models(self):
        if not hasattr(self, "mmdit"):
            self.load_mmdit()
        if not hasattr(self, "decoder") and self._packed_weights is not None and "vae_decoder" in self._packed_weights:
            self.decoder = VAEDecoderEngine(self.vae_config, self._packed_weights["vae_decoder"])
        if self._text_encoder is None:
            self.load_text_encoders()
        if not hasattr(self, "decoder"):
            if isinstance(self.local_ckpt, dict) and "vae_decoder" in self.local_ckpt:
                from .model_io import load_vae_decoder_checkpoint
                named = load_vae_decoder_checkpoint(self.local_ckpt["vae_decoder"], self.vae_config)
            else:
                named = synth_vae_weights(self.vae_config, seed=self.weights_seed + 1, device="cpu")
            self.decoder = VAEDecoderEngine(self.vae_config, pack_vae(self.vae_config, named, self.device))

    def load_vae_encoder(self):
        """The image -> latent half is only needed by img2img (``image_path=``); built on first use
        (mlx/__init__.py:586-588 loads it next to the decoder)."""
        if hasattr(self, "encoder"):
            return
        cfg = self.vae_encoder_config
        if self._packed_weights is not None and "vae_encoder" in self._packed_weights:
            self.encoder = VAEEncoderEngine(cfg, self._packed_weights["vae_encoder"])
            return
        if isinstance(self.local_ckpt, dict) and "vae_encoder" in self.local_ckpt:
            from .model_io import load_vae_encoder_checkpoint
            named = load_vae_encoder_checkpoint(self.local_ckpt["vae_encoder"], cfg)
        else:
            named = synth_vae_encoder_weights(cfg, seed=self.weights_seed + 2, device="cpu")
        self.encoder = VAEEncoderEngine(cfg, pack_vae(cfg, named, self.device))

    # -- text conditioning (outside the hot path) ------------------------------------------------
    def set_text_encoder(self, fn: Callable) -> None:
        """Plug in a callable ``fn(text, cfg_weight, negative_text) -> (conditioning, pooled)``, e.g. a
        ``diffusionkit_amd.text.TextConditioner`` (the reference's CLIP / T5 stack, mlx/__init__.py:176-251)."""
        self._text_encoder = fn

    def load_text_encoders(self) -> bool:
        """Builds the CLIP / T5 engines and tokenizers named in ``local_ckpt`` (there is no hub access here, so nothing is
        downloaded): keys ``clip_l`` / ``clip_g`` / ``t5`` = Hugging Face checkpoint paths (or state dicts),
        ``tokenizer_l`` / ``tokenizer_g`` = (vocab.json, merges.txt), ``t5_tokenizer`` = a local tokenizer directory
        (mlx/__init__.py:119-147, model_io.py:788-962).  Returns False (synthetic conditioning stays) when they are absent."""
        ck = self.local_ckpt if isinstance(self.local_ckpt, dict) else {}
        need = ("clip_l", "tokenizer_l", "t5", "t5_tokenizer") if self._IS_FLUX else ("clip_l", "tokenizer_l", "clip_g", "tokenizer_g")
        if not all(k in ck for k in need):
            return False
        from . import text as tx
        from .model_io import load_clip_checkpoint, load_t5_checkpoint
        clip_l = tx.CLIPTextEngine(tx.CLIP_L, load_clip_checkpoint(ck["clip_l"], tx.CLIP_L), self.device)
        tok_l = tx.Tokenizer.from_files(*ck["tokenizer_l"], pad_with_eos=True)
        t5 = t5_tok = clip_g = tok_g = None
        t5_len = T5_MAX_LENGTH[self.model_version]
        if "t5" in ck and "t5_tokenizer" in ck and self.use_t5:
            t5 = tx.T5EncoderEngine(tx.T5_XXL, load_t5_checkpoint(ck["t5"], tx.T5_XXL), self.device)
            t5_tok = tx.T5Tokenizer(ck["t5_tokenizer"], t5_len)
        if not self._IS_FLUX:
            clip_g = tx.CLIPTextEngine(tx.CLIP_G, load_clip_checkpoint(ck["clip_g"], tx.CLIP_G), self.device)
            tok_g = tx.Tokenizer.from_files(*ck["tokenizer_g"], pad_with_eos=False)
        self.set_text_encoder(tx.TextConditioner(clip_l, tok_l, t5=t5, t5_tokenizer=t5_tok, clip_g=clip_g, tokenizer_g=tok_g,
                                                 flux=self._IS_FLUX, t5_max_length=t5_len))
        return True

    def text_len(self) -> int:
        if self._text_len_override is not None:
            return self._text_len_override
        if self._IS_FLUX:
            return T5_MAX_LENGTH[self.model_version]
        return 77 + (T5_MAX_LENGTH[self.model_version] if self.use_t5 else 77)

    def _synthetic_conditioning(self, text: str, rows: int):
        cfg = self.mmdit_config
        seed = int.from_bytes(hashlib.sha256(text.encode("utf-8")).digest()[:4], "little")
        g = torch.Generator().manual_seed(seed)
        cond = torch.randn(rows, self.text_len(), cfg.token_level_text_embed_dim, generator=g)
        pooled = torch.randn(rows, cfg.pooled_text_embed_dim, generator=g)
        return cond.to(self.device, torch.bfloat16), pooled.to(self.device, torch.bfloat16)

    def encode_text(self, text: str, cfg_weight: float = 7.5, negative_text: str = ""):
        """mlx/__init__.py:197-251: returns (conditioning [2,S_t,4096], pooled [2,2048]); row 0 is the
        prompt, row 1 the negative prompt (always present)."""
        if self._text_encoder is not None:
            return self._text_encoder(text, cfg_weight, negative_text)
        c0, p0 = self._synthetic_conditioning(text, 1)
        c1, p1 = self._synthetic_conditioning("\0neg:" + negative_text, 1)
        return torch.cat([c0, c1], 0), torch.cat([p0, p1], 0)

    # -- hot path -----------------------------------------------------------------------------
    def denoise_latents(
        self,
        conditioning,
        pooled_conditioning,
        num_steps: int = 2,
        cfg_weight: float = 0.0,
        latent_size: Tuple[int, int] = (64, 64),
        seed=None,
        image_path: Optional[str] = None,
        denoise: float = 1.0,
        *,
        mask_path=None,
        block_cache=None,
        sampler=None,
        sampler_eta=None,
        guidance=None,
        guidance_rescale: float = 0.7,
        apg_eta: float = 0.0,
        apg_norm_threshold: float = 0.0,
        apg_momentum: float = 0.0,
        guidance_interval=None,
        reference_image_path=None,
        condition_image_path=None,
        condition_mask_path=None,
        skip_layer_guidance=None,
        skip_layers=None,
        skip_layer_interval=None,
        pag_scale=None,
        pag_layers=None,
        pag_interval=None,
        controlnet_image_path=None,
        controlnet_scale: float = 1.0,
        controlnet_interval=None,
        ip_adapter_image_embeds=None,
        ip_adapter_scale: float = 1.0,
        edit_source_text=None,
        edit_steps=None,
        edit_n_avg=None,
        edit_source_cfg=None,
    ):
        """``edit_source_text`` (FlowEdit, Kulikov et al. 2024; text-guided editing of ``image_path`` with the plain checkpoint): the prompt that
        describes the source image -- a string, encoded here with ``encode_text``, or an already encoded (conditioning, pooled_conditioning) pair
        laid out like this call's own -- while ``conditioning`` describes what the image should become.  See ``_denoise_edit`` for ``edit_steps`` =
        (n_max, n_min), ``edit_n_avg`` and ``edit_source_cfg``, what it composes with and what it refuses.  ``self.last_edit`` says what ran; None
        without the option, and then every launch and every bit is what it was.
        ``ip_adapter_image_embeds`` (a pipeline built with ``ip_adapter_ckpt``; an array or tensor [E], [n, E] with n = 1 or one row per seed, or a
        list with one [E] per seed): the prepared image embedding(s) of the image prompt -- CLIP ViT-L/14 ``image_embeds``, diffusers'
        ``ip_adapter_image_embeds=``; the vision tower is not part of this build.  They are projected to the adapter's tokens once per call
        (``engine.ip_adapter_project``), every double block's keys and values are cached (``MMDiTEngine.cache_ip_tokens``), and every model evaluation
        adds ``ip_adapter_scale`` times the decoupled attention's output behind each double block.  Scale 0 runs the plain launches.  Composes with
        seed lists, every sampler, img2img and ``mask_path``.  Raises on ``cfg_weight > 0`` (negative image embeds are not built), ``block_cache``,
        a reference image, on these keywords without an adapter and on their absence with one.  ``self.last_ip_adapter`` = {"scale", "tokens",
        "images"}, or None.
        ``controlnet_image_path`` (a pipeline built with ``controlnet_ckpt``; a path, a PIL image or an array, or a list with one per seed): the
        prepared control image (edges, pose, ...) at the OUTPUT size -- never resized, sides multiples of 16 -- VAE-encoded to the posterior's mean (the
        published pipeline samples), put through the latent format's ``process_in`` and patchified.  Every model evaluation of a controlled step first
        runs the ControlNet's engine on the same tokens, both CFG rows included, and the main engine adds ``controlnet_scale`` times its taps
        (``MMDiTEngine.set_control_taps``).  ``controlnet_interval`` = (start, stop): step i of n is controlled iff i / n >= start and
        (i + 1) / n <= stop (diffusers' control_guidance_start / _end; Heun's two evaluations share their step's decision); outside it the ControlNet
        is not run and the launches are the plain ones.  Composes with seed lists, every sampler and guidance mode, ``guidance_interval`` (both
        engines are re-prepared together), img2img, inpainting and float16.  Raises on ``block_cache``, skip-layer and perturbed-attention guidance,
        on these keywords without a ControlNet and on their absence with one.  ``self.last_controlnet`` = {"scale", "interval", "evals"}, or None.
        mlx/__init__.py:253-292.  ``seed`` may be a list: one image per seed is denoised in a
        single batched step loop (data-parallel sharding hands each rank a list).
        ``mask_path`` (inpainting; a path, a PIL image or an array as ``read_mask`` takes them, or a list with one per seed): repaint where the
        mask is 255, keep ``image_path``'s content where it is 0 -- kept latent cells equal the encoded image bit for bit.
        ``block_cache`` (first-block cache; a float threshold >= 0 or a policy object with ``decide(step, n_steps, rel)``, see
        ``sampler.BlockCachePolicy``): every step runs block 0, and where its effect on the image rows moved by less than the threshold,
        relative to the last computed step, the cached effect of the other blocks is reused instead of running them.  One decision per launch:
        the images of a seed list and the two CFG rows share it through the maximum of their changes, so a cached batch equals the single
        runs only where their decisions coincide.  What was decided is kept in ``self.last_block_cache`` (threshold, computed and skipped
        steps, rel per step; None without the option).  No threshold has been validated on a real checkpoint here.
        ``sampler``: None or "euler" (the reference's first-order loop, today's launches and bits), "heun" (second order, two model evaluations
        per step but the last) or "ab2" (second order, one evaluation per step, the previous step's direction kept in an fp32 buffer); every
        composition above works with them, except that "heun" refuses ``block_cache`` (see ``sample_steps``).  ``self.last_sampler`` says what
        ran: {"sampler", "model_evals"}.  Their order is checked on an analytic problem (profiles/samplers.md), not on a trained checkpoint.
        Stochastic samplers: "euler_a" (k-diffusion's sample_euler_ancestral_RF; ``sampler_eta`` in [0, 1], default 1, the share of the step that is
        re-noised: 0 is "euler", its launches and its bits) and "sde" (diffusers' FlowMatchEulerDiscreteScheduler(stochastic_sampling=True): x' =
        (1 - sigma') den + sigma' xi, all of the noise re-drawn every step -- offered as the published definition and nothing more: at a finite number
        of steps it does not preserve the marginals of a mean-predicting denoiser, profiles/stochastic_samplers.md).  First order, one evaluation per
        step.  The noise is drawn inside the step launch (dk_noisy_cfg_step) from a counter: Philox4x32-10 keyed by the image's own seed -- the one its
        start noise was drawn with; with ``seed=None`` the one picked and logged here -- at the schedule index of the step, so an image's result depends
        on its seed alone, not on its place in a seed list, the batch size, CFG or the element type; a schedule cut by ``denoise`` keeps the draws of
        the entries it keeps.  The seeds are uploaded once per call.  The rows go through the same loop as every plan, so the compositions above hold
        (inpainting: the blend still re-noises the known region with the start draw).  ``sampler_eta`` with any other sampler raises.
        ``self.last_sampler`` then also holds "eta" (None under "sde") and "noise_draws", the number of launches that drew noise.  Arithmetic only, on
        synthetic weights: nothing here says anything about image quality on a trained checkpoint.
        ``guidance`` (models with ``cfg_weight > 0``): None or "cfg" (neg + w (pos - neg), today's launches and bits), "rescale" (the same, scaled by
        ``guidance_rescale`` * std(pos) / std(cfg) + 1 - ``guidance_rescale`` per image) or "apg" (adaptive projected guidance on the x0 predictions:
        ``apg_eta`` weighs the component parallel to the prompt prediction, ``apg_norm_threshold`` > 0 clips the norm of the direction per image,
        ``apg_momentum`` carries it over the guided evaluations in an fp32 buffer); the definitions are ``sampler.guide_reference``'s.
        ``guidance_interval`` = (lo, hi): only evaluations with lo <= sigma <= hi are guided; the others run the prompt rows alone, the engine
        re-prepared for half the batch at every change.  Any of these options goes through ``sample_steps`` (Euler as its plan) and raises with
        ``cfg_weight <= 0``.  ``self.last_guidance`` says what ran: the mode, its parameters, the interval and the guided / unguided evaluation
        counts.  The modes are verified as arithmetic only: no setting has been validated on a trained checkpoint here.
        ``reference_image_path`` (reference-image conditioning in FLUX.1 Kontext's token layout, FLUX family only; a path, a PIL image or an array,
        or a list with one per seed; sides multiples of 16 pixels, never resized): the image is encoded to the VAE posterior's mean, goes through
        ``latent_format.process_in`` and rides behind the image tokens of every model evaluation at RoPE index 1 (``MMDiTEngine.cache_reference``,
        embedded once per call).  It composes with every option above.  ``self.last_reference`` = {"size": (H, W), "tokens": S_r}, or None
        without the option.  Verified as arithmetic only: no Kontext checkpoint has been run here.
        ``condition_image_path`` / ``condition_mask_path`` (channel-concatenated conditioning, ``FluxPipeline(condition="fill" | "control")``; a path, a
        PIL image or an array, or a list with one per seed; sides equal to the output's, never resized): the published FLUX sampling code's
        ``prepare_fill`` / ``prepare_control``.  "control": the prepared control image (edges, depth) is VAE-encoded, goes through ``process_in`` and
        its 64 patch features are concatenated to the latent's in every model evaluation.  "fill": the image times (1 - mask / 255) is encoded the same
        way, and 256 more columns carry the mask itself (not binarised; 255 = repaint).  The encoder's posterior MEAN is taken where the published code
        samples, so the same inputs give the same conditioning whatever the seed.  The condition's share of x_embedder is computed once per call
        (``MMDiTEngine.cache_condition``); the step loop and every option above are untouched.  Refused before any GPU work: the keywords on a
        pipeline without ``condition``, a ``condition`` pipeline without them, "fill" without a mask, "control" with one, a reference image at the same
        time, the SD3 family.  ``self.last_condition`` = {"kind", "features"}, or None.  Verified as arithmetic only: no Fill / Canny / Depth checkpoint
        has been run here.
        ``skip_layer_guidance`` (skip-layer guidance, SD3 family with ``cfg_weight > 0``; None: off): the scale s of a third evaluation per step, the
        prompt rows through a model that skips the double blocks ``skip_layers``: den = G(pos, neg) + s (pos - skip), G the guidance mode's combination
        (``sampler.slg_reference``).  Step i of n takes the term iff n start < i < n stop, ``skip_layer_interval`` = (start, stop), and only in
        evaluations a ``guidance_interval`` leaves guided.  The third evaluation rides as a third row group of the same launches: it joins in front
        of the first skipped block and sits out the skipped ones, so it costs the blocks it runs; the engine is re-prepared where the group count
        changes (twice for one window).  ``skip_layers`` / ``skip_layer_interval`` None take the defaults published with the model version
        (``config.SKIP_LAYER_GUIDANCE``: SD3.5-medium (7, 8, 9) and (0.01, 0.2); ``skip_layer_guidance=True`` takes its scale, 2.5, too); any other
        version must name its layers, and its interval defaults to (0, 1).  Composes with seed lists, every sampler and guidance mode, img2img,
        inpainting and float16.  Raises on FLUX, ``cfg_weight <= 0``, ``block_cache`` (no cache policy for a forked row group yet) and a layer outside
        the model.  ``self.last_skip_layer_guidance`` = {"layers", "scale", "interval", "evals"} (evaluations with the term), or None.  Verified as
        arithmetic only, on synthetic weights: no SD3.5-medium checkpoint has been run here.
        ``pag_scale`` (perturbed-attention guidance, diffusers' StableDiffusion3PAGPipeline; SD3 family with ``cfg_weight > 0``; None: off): the scale
        s of a third evaluation, the prompt rows through a model whose double blocks ``pag_layers`` run their attention perturbed -- image queries
        attend to the text keys and to their own key only: den = G(pos, neg) + s (pos - perturbed), the same term and the same step launch as
        skip-layer guidance.  ``pag_interval`` None: every guided evaluation carries it; (start, stop): step i of n iff n start < i < n stop.  There
        is no published recipe: scale and layers come together.  The third row group is forked inside the engine
        (``MMDiTEngine.set_perturbed_attention``).  Composes with seed lists, every sampler and guidance mode, ``guidance_interval``, img2img,
        inpainting and float16.  Raises on FLUX, ``cfg_weight <= 0``, ``block_cache``, an fp8 engine, a reference image, a condition and together
        with skip-layer guidance (there is one fork).  ``self.last_perturbed_attention_guidance`` = {"layers", "scale", "interval", "evals"}, or
        None.  Verified as arithmetic only, on synthetic weights: no checkpoint has been run here."""
        self.last_edit = None
        if edit_source_text is None:
            if edit_steps is not None or edit_n_avg is not None or edit_source_cfg is not None:
                raise ValueError("edit_steps, edit_n_avg and edit_source_cfg belong to an edit: give edit_source_text, the prompt that describes image_path")
        else:
            refused = {"mask_path (inpainting)": mask_path, "block_cache": block_cache,
                       "a guidance mode other than 'cfg'": None if guidance in (None, "cfg") else guidance, "guidance_interval": guidance_interval,
                       "skip-layer guidance": next((v for v in (skip_layer_guidance, skip_layers, skip_layer_interval) if v is not None), None),
                       "perturbed-attention guidance": next((v for v in (pag_scale, pag_layers, pag_interval) if v is not None), None),
                       "a ControlNet": controlnet_image_path if controlnet_image_path is not None else getattr(self, "controlnet", None),
                       "an IP-Adapter": ip_adapter_image_embeds if ip_adapter_image_embeds is not None else getattr(self, "ip_adapter_config", None),
                       "a reference image": reference_image_path,
                       "channel-concatenated conditioning (condition=)": condition_image_path if condition_image_path is not None
                       else getattr(self, "condition", None)}
            for what, value in refused.items():
                if value is not None:
                    raise ValueError(_flowedit_refusal(what))
            if denoise != 1.0:
                raise ValueError("an edit (edit_source_text) cannot run together with denoise (img2img strength): the edit starts from the image itself, "
                                 "and edit_steps = (n_max, n_min) says which part of the schedule it covers")
            return self._denoise_edit(conditioning, pooled_conditioning, num_steps, cfg_weight, seed, image_path, sampler, sampler_eta, edit_source_text,
                                      edit_steps, edit_n_avg, edit_source_cfg)
        check_condition_args(getattr(self, "condition", None), condition_image_path, condition_mask_path, reference_image_path, self._IS_FLUX)
        if reference_image_path is not None and not self._IS_FLUX:
            raise ValueError(_REFERENCE_NEEDS_ROPE)
        slg = None
        if skip_layer_guidance is not None or skip_layers is not None or skip_layer_interval is not None:
            slg = _skip_layer_options(skip_layer_guidance, skip_layers, skip_layer_interval, self.model_version, self.mmdit_config, self._IS_FLUX,
                                      cfg_weight, block_cache)
        pag = None
        if pag_scale is not None or pag_layers is not None or pag_interval is not None:
            pag = _perturbed_attention_options(pag_scale, pag_layers, pag_interval, self.mmdit_config, self._IS_FLUX, cfg_weight, block_cache,
                                               reference_image_path, getattr(self, "condition", None) or condition_image_path, slg)
        guide = _guidance_options(guidance, guidance_rescale, apg_eta, apg_norm_threshold, apg_momentum, guidance_interval, cfg_weight)
        if mask_path is not None and image_path is None:
            raise ValueError("mask_path needs image_path: the mask says which part of that image to keep")
        n_seeds = len(seed) if isinstance(seed, (list, tuple)) else 1
        control = _controlnet_options(self, controlnet_image_path, controlnet_scale, controlnet_interval, n_seeds,
                                      (latent_size[0] * 8, latent_size[1] * 8) if image_path is None else read_image_u8(image_path).shape[:2],
                                      block_cache, slg, pag, reference_image_path,
                                      getattr(self, "condition", None) or condition_image_path)  # (raises before any GPU work)
        ip = _ip_adapter_options(self, ip_adapter_image_embeds, ip_adapter_scale, n_seeds, cfg_weight, block_cache, reference_image_path)
        sampler = check_sampler(sampler)
        eta = check_sampler_eta(sampler, sampler_eta)
        if sampler == "heun" and block_cache is not None:
            raise ValueError(_HEUN_BLOCK_CACHE)
        seed = int(time.time()) if seed is None else seed
        seeds = list(seed) if isinstance(seed, (list, tuple)) else [seed]
        logger.info(f"Seed: {seeds}")
        refs = None if reference_image_path is None else _read_references(reference_image_path, len(seeds))  # (raises before any GPU work)
        cond_px = None
        if condition_image_path is not None:  # (the same)
            out_hw = (latent_size[0] * 8, latent_size[1] * 8) if image_path is None else read_image_u8(image_path).shape[:2]  # (img2img: the image's)
            cond_px = read_condition_images(condition_image_path, condition_mask_path, out_hw, len(seeds))
        x_T = self.get_empty_latent(*latent_size)
        if image_path is None:
            denoise = 1.0
            x_T = np.repeat(x_T, len(seeds), axis=0) if len(seeds) > 1 else x_T
        else:
            # img2img (mlx/__init__.py:270-277): the encoded image, one posterior sample per seed
            x_orig = torch.cat([self.latent_format.process_in(self.encode_image_to_latents(image_path, seed=s)) for s in seeds], 0)
            x_T = x_orig.cpu().numpy()
        noise = np.concatenate([self.get_noise(s, x_T[:1]) for s in seeds], axis=0)
        sigmas = self.get_sigmas(self.sampler, num_steps)
        cut = int(num_steps * (1 - denoise))
        sigmas = sigmas[cut:]
        extra_args = {
            "conditioning": conditioning,
            "cfg_weight": cfg_weight,
            "pooled_conditioning": pooled_conditioning,
        }
        if mask_path is not None:
            from . import ops
            hl, wl = x_T.shape[1:3]
            masks = _read_masks(mask_path, (hl * 8, wl * 8), len(seeds))
            extra_args["mask"] = ops.mask_to_latent(torch.from_numpy(masks).to(self.device), 8)
            extra_args["x_orig"] = x_orig
            extra_args["noise"] = torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float32)).to(self.device)
        if block_cache is not None:
            extra_args["block_cache"] = block_cache
        if guide is not None:
            extra_args["guidance"] = guide
        if slg is not None:
            extra_args["skip_layer_guidance"] = slg
        if pag is not None:
            extra_args["perturbed_attention_guidance"] = pag
        if control is not None:
            z = self.latent_format.process_in(self.encode_reference_to_latents(control["pixels"]))
            if self.controlnet.config.guidance_embed:  # (a guidance-distilled FLUX ControlNet sees the strength the model sees)
                self.controlnet.guidance = self.mmdit.guidance
            extra_args["controlnet"] = {"engine": self.controlnet, "tokens": self.controlnet.patchify(z.to(torch.float32).contiguous()),
                                        "scale": control["scale"], "interval": control["interval"]}
        self.last_ip_adapter = None
        if ip is not None:
            from .engine import ip_adapter_project
            ipc = self.ip_adapter_config
            extra_args["ip_adapter"] = {"tokens": ip_adapter_project(self.mmdit.weights, ipc, torch.from_numpy(ip["embeds"])), "scale": ip["scale"]}
            self.last_ip_adapter = {"scale": ip["scale"], "tokens": ipc.ip_adapter_tokens, "images": int(ip["embeds"].shape[0])}
        self.last_reference = None
        if refs is not None:
            extra_args["reference"] = self.latent_format.process_in(self.encode_reference_to_latents(refs))
            p = self.mmdit_config.patch_size
            self.last_reference = {"size": tuple(refs.shape[1:3]), "tokens": (refs.shape[1] // (8 * p)) * (refs.shape[2] // (8 * p))}
        self.last_condition, self._condition_pixels = None, None
        if cond_px is not None:
            extra_args["condition"] = self.condition_tokens(*cond_px)
            self.last_condition = {"kind": self.condition, "features": int(extra_args["condition"].shape[-1])}
            self._condition_pixels = cond_px
        noise_scaled = self.sampler.noise_scaling(np.float32(sigmas[0]), noise, x_T, self.max_denoise(sigmas))
        x0 = torch.from_numpy(np.ascontiguousarray(noise_scaled, dtype=np.float32)).to(self.device)
        denoiser = CFGDenoiser(self)
        stochastic = sampler in STOCHASTIC_SAMPLERS
        rows = "euler" if sampler == "euler_a" and eta == 0.0 else sampler  # (eta = 0: euler's rows, and so euler's launches)
        try:
            if rows == "euler" and guide is None and slg is None and pag is None:
                latent, iter_time = sample_euler(denoiser, x0, sigmas, extra_args=extra_args)
                evals, draws = len(iter_time), 0
            else:
                plan = step_plan(rows, sigmas, eta if rows == "euler_a" else None, first_draw=cut)
                draws = sum(r.cn != 0.0 for r in plan)
                if draws:  # (the seeds the start noise was drawn with, one per image)
                    extra_args["noise_seeds"] = [int(s) for s in seeds]
                latent, iter_time = sample_steps(denoiser, x0, sigmas, plan, extra_args=extra_args)
                evals = len(plan)
        finally:
            if ip is not None:  # (the engine outlives the call: off again, the plain launches)
                self.mmdit.set_ip_scale(0.0)
        self.last_sampler = {"sampler": sampler, "model_evals": evals}
        if stochastic:  # (keys of the stochastic samplers alone)
            self.last_sampler.update(eta=eta if sampler == "euler_a" else None, noise_draws=draws)
        self.last_block_cache = denoiser.block_cache_record
        self.last_guidance = denoiser.guidance_record or dict(_DEFAULT_GUIDANCE, guided_evals=evals if cfg_weight > 0 else 0,
                                                              unguided_evals=0 if cfg_weight > 0 else evals)
        self.last_skip_layer_guidance = denoiser.skip_layer_record
        self.last_perturbed_attention_guidance = denoiser.perturbed_attention_record
        self.last_controlnet = denoiser.controlnet_record
        latent = self.latent_format.process_out(latent)
        return latent, iter_time

    def _denoise_edit(self, conditioning, pooled_conditioning, num_steps, cfg_weight, seed, image_path, sampler, sampler_eta, source, edit_steps,
                      n_avg, source_cfg):
        """``denoise_latents`` under ``edit_source_text``: FlowEdit.  ``image_path`` (a path, a PIL image or an array, or a list with one per seed) is
        VAE-encoded to the posterior's MEAN, as Fill and Kontext take it, and put through ``process_in``: that is x_src, and the latent size is the
        image's.  Z starts there and takes, for the steps T - n_max .. T - n_min - 1 of the ``num_steps`` = T schedule, (sigma' - sigma) times the
        mean over ``edit_n_avg`` draws of V(Zt, target) - V(Zs, source), Zs = (1 - sigma) x_src + sigma xi and Zt = Zs + (Z - x_src)
        (``sample_flowedit``; the definition is ``sampler.flowedit_reference``).  With n_min > 0 one more draw forms Zt at sigmas[T - n_min], and
        the ordinary loop -- whatever ``sampler`` names -- takes it to sigma 0 with the target conditioning alone.
        ``edit_steps`` = (n_max, n_min) with 0 <= n_min < n_max <= num_steps; ``edit_n_avg`` >= 1 (default 1).  ``edit_source_cfg``: the source's CFG
        weight on the SD3 family (``cfg_weight`` is the target's; both must be positive), the source's distilled-guidance value on FLUX.1-dev
        (``self.mmdit.guidance`` is the target's: the engine then embeds one value per batch row); refused on a FLUX model without a guidance
        embedding (FLUX.1-schnell).  Defaults, ``sampler.FLOWEDIT_DEFAULTS``, are the paper's settings AS RECALLED and have NOT been verified against
        the paper or the authors' code: n_max = 33 of T = 50 with source 3.5 / target 13.5 (SD3), n_max = 24 of T = 28 with 1.5 / 5.5 (FLUX.1-dev);
        without ``edit_steps`` n_max is that share of ``num_steps``, rounded, and n_min 0.
        The noise is drawn inside the step launch from Philox keyed by each image's seed (stream tag 1; a stochastic sampler in the tail draws
        on tag 0), so a result depends on its seed alone: a seed list gives each image the bits of its single-seed run.  Composes with seed lists
        (one image for all seeds, or one per seed), both families, CFG and float16; fp8 engines take the same launches, untested beyond
        construction.  ``self.last_edit`` = {"n_max", "n_min", "n_avg", "model_evals", "draws", "rows", "source_cfg", "target_cfg",
        "guidance_rows", "tail_evals"}.  Arithmetic only, on synthetic weights: nothing here says anything about image quality."""
        from .sampler import FLOWEDIT_DEFAULTS, check_flowedit
        if image_path is None:
            raise ValueError("an edit (edit_source_text) needs image_path: the image to edit")
        family = "flux" if self._IS_FLUX else "sd3"
        t_ref, nmax_ref, nmin_ref, src_ref, _ = FLOWEDIT_DEFAULTS[family]
        if edit_steps is None:
            edit_steps = (max(1, min(int(num_steps), round(num_steps * nmax_ref / t_ref))), nmin_ref)
        if len(tuple(edit_steps)) != 2:
            raise ValueError(f"edit_steps must be (n_max, n_min), got {edit_steps!r}")
        n_max, n_min, n_avg = check_flowedit(num_steps, edit_steps[0], edit_steps[1], 1 if n_avg is None else n_avg)
        cfg_on = cfg_weight > 0
        guided_model = bool(self.mmdit_config.guidance_embed)
        grow_values = None
        if self._IS_FLUX:
            if source_cfg is not None and not guided_model:
                raise ValueError("edit_source_cfg on the FLUX family is the source's distilled-guidance value: this model has no guidance embedding "
                                 "(FLUX.1-schnell)")
            w_src = float(cfg_weight)
            if guided_model:
                grow_values = (float(src_ref if source_cfg is None else source_cfg), float(self.mmdit.guidance))
        else:
            w_src = float(src_ref if source_cfg is None else source_cfg)
            if not cfg_on or not w_src > 0:
                raise ValueError("an edit on the SD3 family needs classifier-free guidance on both sides (cfg_weight > 0 and edit_source_cfg > 0)")
        sampler = check_sampler(sampler)
        eta = check_sampler_eta(sampler, sampler_eta)
        seed = int(time.time()) if seed is None else seed
        seeds = [int(s) for s in (seed if isinstance(seed, (list, tuple)) else [seed])]
        logger.info(f"Seed: {seeds}")
        n = len(seeds)
        images = list(image_path) if isinstance(image_path, (list, tuple)) else [image_path]
        if len(images) not in (1, n):
            raise ValueError(f"{len(images)} source images for {n} seeds: give one image, or one per seed")
        if isinstance(source, str):
            source = self.encode_text(source, cfg_weight, "")
        src_c, src_p = source
        if src_c.dim() == 4:
            src_c = src_c.squeeze(2)
        if conditioning.dim() == 4:
            conditioning = conditioning.squeeze(2)
        tar_c, tar_p = _tile_conditioning(conditioning, pooled_conditioning, n, cfg_on, self._IS_FLUX)
        src_c, src_p = _tile_conditioning(src_c, src_p, n, cfg_on, self._IS_FLUX)
        rows = n * (2 if cfg_on else 1)
        for what, t in (("conditioning", tar_c), ("edit_source_text", src_c)):
            if t.shape[0] != rows:
                raise ValueError(f"{what} has {t.shape[0]} rows for {n} images{' with CFG' if cfg_on else ''}: expected {rows}")
        if src_c.shape[1:] != tar_c.shape[1:]:
            raise ValueError(f"the source conditioning {tuple(src_c.shape)} and the target conditioning {tuple(tar_c.shape)} differ in length or width")
        # [src | tar], or [src+ | tar+ | src- | tar-]: 2 n images whose rows are laid out per image
        pair = lambda a, b: torch.cat([t.to(self.device) for k in range(0, rows, n) for t in (a[k:k + n], b[k:k + n])], 0)  # noqa: E731
        x_src = torch.cat([self.latent_format.process_in(self.encode_mean_latents(self.read_image(im))) for im in images], 0)
        if len(images) == 1 and n > 1:
            x_src = x_src.expand(n, *x_src.shape[1:])
        x_src = x_src.to(torch.float32).contiguous()
        sigmas = self.get_sigmas(self.sampler, num_steps)
        denoiser = CFGDenoiser(self)
        extra_args = {"conditioning": pair(src_c, tar_c), "pooled_conditioning": pair(src_p, tar_p), "cfg_weight": cfg_weight, "noise_seeds": seeds,
                      "edit_source_cfg": w_src}
        if grow_values is not None:
            extra_args["edit_guidance_rows"] = [g for _ in range(0, rows, n) for g in grow_values for _ in range(n)]
        z, zt, iter_time = sample_flowedit(denoiser, x_src, sigmas, n_max, n_min, n_avg, extra_args=extra_args)
        record = dict(denoiser.flowedit_record, tail_evals=0)
        latent, evals, draws = z, record["model_evals"], 0
        stochastic = sampler in STOCHASTIC_SAMPLERS
        if n_min > 0:  # the paper's "regular sampling" tail: the ordinary loop on the cut schedule, the target rows alone
            cut = int(num_steps) - n_min
            tail_args = {"conditioning": tar_c, "pooled_conditioning": tar_p, "cfg_weight": cfg_weight}
            rows_name = "euler" if sampler == "euler_a" and eta == 0.0 else sampler
            if rows_name == "euler":
                latent, tail_time = sample_euler(denoiser, zt, sigmas[cut:], extra_args=tail_args)
                tail_evals = len(tail_time)
            else:
                plan = step_plan(rows_name, sigmas[cut:], eta if rows_name == "euler_a" else None, first_draw=cut)
                draws = sum(r.cn != 0.0 for r in plan)
                if draws:
                    tail_args["noise_seeds"] = seeds
                latent, tail_time = sample_steps(denoiser, zt, sigmas[cut:], plan, extra_args=tail_args)
                tail_evals = len(plan)
            iter_time = iter_time + tail_time
            evals += tail_evals
            record.update(tail_evals=tail_evals, model_evals=evals)
        self.last_edit = record
        self.last_sampler = {"sampler": sampler, "model_evals": evals}
        if stochastic:
            self.last_sampler.update(eta=eta if sampler == "euler_a" else None, noise_draws=draws)
        self.last_block_cache = None
        self.last_guidance = dict(_DEFAULT_GUIDANCE, guided_evals=evals if cfg_on else 0, unguided_evals=0 if cfg_on else evals)
        self.last_skip_layer_guidance = self.last_perturbed_attention_guidance = self.last_controlnet = None
        self.last_ip_adapter = self.last_reference = self.last_condition = None
        return self.latent_format.process_out(latent), iter_time

    def generate_image(
        self,
        text: str,
        num_steps: int = 2,
        cfg_weight: float = 0.0,
        negative_text: str = "",
        latent_size: Tuple[int, int] = (64, 64),
        seed=None,
        verbose: bool = True,
        image_path: Optional[str] = None,
        denoise: float = 1.0,
        *,
        mask_path=None,
        composite: bool = True,
        block_cache=None,
        sampler=None,
        sampler_eta=None,
        guidance=None,
        guidance_rescale: float = 0.7,
        apg_eta: float = 0.0,
        apg_norm_threshold: float = 0.0,
        apg_momentum: float = 0.0,
        guidance_interval=None,
        reference_image_path=None,
        condition_image_path=None,
        condition_mask_path=None,
        skip_layer_guidance=None,
        skip_layers=None,
        skip_layer_interval=None,
        pag_scale=None,
        pag_layers=None,
        pag_interval=None,
        controlnet_image_path=None,
        controlnet_scale: float = 1.0,
        controlnet_interval=None,
        ip_adapter_image_embeds=None,
        ip_adapter_scale: float = 1.0,
        edit_source_text=None,
        edit_steps=None,
        edit_n_avg=None,
        edit_source_cfg=None,
    ):
        """``edit_source_text``, ``edit_steps``, ``edit_n_avg``, ``edit_source_cfg``: FlowEdit, text-guided editing of ``image_path`` -- ``text`` says
        what the image should become, ``edit_source_text`` what it shows now; see ``denoise_latents``.  ``log["denoising"]["edit"]`` is
        ``self.last_edit``.
        ``ip_adapter_image_embeds``, ``ip_adapter_scale``: FLUX IP-Adapter, see ``denoise_latents``; ``log["denoising"]["ip_adapter"]`` is
        ``self.last_ip_adapter``.
        ``controlnet_image_path``, ``controlnet_scale``, ``controlnet_interval``: SD3 ControlNet, see ``denoise_latents``; with a ControlNet,
        ``log["denoising"]["controlnet"]`` is ``self.last_controlnet``.
        mlx/__init__.py:294-534: returns (PIL.Image, log).  ``mask_path``: inpainting, see ``denoise_latents``; with ``composite`` the pixels
        the mask keeps are pasted back from the input image after decoding (the VAE round trip alone does not reproduce them).
        ``block_cache``: first-block cache, see ``denoise_latents``; its record goes to ``log["denoising"]["block_cache"]``.
        ``sampler``: "euler" (default) | "heun" | "ab2" | "euler_a" | "sde", see ``denoise_latents``; ``log["denoising"]["sampler"]`` and
        ``["model_evals"]`` say what ran, under the stochastic samplers (``sampler_eta``: euler_a's eta) also ``["eta"]`` and ``["noise_draws"]``.
        ``guidance``, ``guidance_rescale``, ``apg_eta``, ``apg_norm_threshold``, ``apg_momentum``, ``guidance_interval``: see ``denoise_latents``; with any
        of them set, ``log["denoising"]["guidance"]`` is ``self.last_guidance``.
        ``reference_image_path``: reference-image conditioning, see ``denoise_latents``; with it set, ``log["denoising"]["reference"]`` is
        ``self.last_reference``.
        ``condition_image_path`` / ``condition_mask_path``: channel-concatenated conditioning, see ``denoise_latents``; ``log["denoising"]["condition"]`` is
        ``self.last_condition``.  With ``composite`` and no ``mask_path``, the pixels a fill mask keeps are pasted back from the condition image.
        ``skip_layer_guidance``, ``skip_layers``, ``skip_layer_interval``: skip-layer guidance, see ``denoise_latents``; with it on,
        ``log["denoising"]["skip_layer_guidance"]`` is ``self.last_skip_layer_guidance``.
        ``pag_scale``, ``pag_layers``, ``pag_interval``: perturbed-attention guidance, see ``denoise_latents``; with it on,
        ``log["denoising"]["perturbed_attention_guidance"]`` is ``self.last_perturbed_attention_guidance``."""
        check_condition_args(getattr(self, "condition", None), condition_image_path, condition_mask_path, reference_image_path, self._IS_FLUX)
        if mask_path is not None and image_path is None:
            raise ValueError("mask_path needs image_path: the mask says which part of that image to keep")
        assert latent_size[0] % 2 == 0, f"Height must be divisible by 16 ({latent_size[0]*8}/16={latent_size[0]/2})"
        assert latent_size[1] % 2 == 0, f"Width must be divisible by 16 ({latent_size[1]*8}/16={latent_size[1]/2})"
        self.check_and_load_models()
        start_time = time.time()
        dev = self.device

        def mem():
            return {"peak_memory": round(bytes2gigabytes(torch.cuda.max_memory_allocated(dev)), 3),
                    "active_memory": round(bytes2gigabytes(torch.cuda.memory_allocated(dev)), 3)}

        log = {
            "text_encoding": {"pre": mem(), "post": {"peak_memory": None, "active_memory": None}},
            "denoising": {"pre": {"peak_memory": None, "active_memory": None}, "post": {"peak_memory": None, "active_memory": None}},
            "decoding": {"pre": {"peak_memory": None, "active_memory": None}, "post": {"peak_memory": None, "active_memory": None}},
            "peak_memory": 0.0,
        }
        t0 = time.time()
        conditioning, pooled_conditioning = self.encode_text(text, cfg_weight, negative_text)
        edit_source = None if edit_source_text is None else self.encode_text(edit_source_text, cfg_weight, negative_text)
        torch.cuda.synchronize(dev)
        log["text_encoding"]["post"] = mem()
        log["text_encoding"]["time"] = round(time.time() - t0, 3)
        log["text_encoding"]["synthetic"] = self._text_encoder is None
        log["peak_memory"] = max(log["peak_memory"], log["text_encoding"]["post"]["peak_memory"])

        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.time()
        log["denoising"]["pre"] = mem()
        latents, iter_time = self.denoise_latents(
            conditioning, pooled_conditioning, num_steps=num_steps, cfg_weight=cfg_weight,
            latent_size=latent_size, seed=seed, image_path=image_path, denoise=denoise, mask_path=mask_path, block_cache=block_cache,
            sampler=sampler, guidance=guidance, guidance_rescale=guidance_rescale, apg_eta=apg_eta, apg_norm_threshold=apg_norm_threshold,
            apg_momentum=apg_momentum, guidance_interval=guidance_interval, **({} if sampler_eta is None else {"sampler_eta": sampler_eta}),
            **({} if reference_image_path is None else {"reference_image_path": reference_image_path}),
            **({} if condition_image_path is None else {"condition_image_path": condition_image_path, "condition_mask_path": condition_mask_path}),
            **({} if skip_layer_guidance is None and skip_layers is None and skip_layer_interval is None else
               {"skip_layer_guidance": skip_layer_guidance, "skip_layers": skip_layers, "skip_layer_interval": skip_layer_interval}),
            **({} if pag_scale is None and pag_layers is None and pag_interval is None else
               {"pag_scale": pag_scale, "pag_layers": pag_layers, "pag_interval": pag_interval}),
            **({} if controlnet_image_path is None and controlnet_interval is None and controlnet_scale == 1.0 and getattr(self, "controlnet", None) is None
               else {"controlnet_image_path": controlnet_image_path, "controlnet_scale": controlnet_scale, "controlnet_interval": controlnet_interval}),
            **({} if ip_adapter_image_embeds is None and ip_adapter_scale == 1.0 and getattr(self, "ip_adapter_config", None) is None
               else {"ip_adapter_image_embeds": ip_adapter_image_embeds, "ip_adapter_scale": ip_adapter_scale}),
            **({} if edit_source_text is None and edit_steps is None and edit_n_avg is None and edit_source_cfg is None else
               {"edit_source_text": edit_source, "edit_steps": edit_steps, "edit_n_avg": edit_n_avg, "edit_source_cfg": edit_source_cfg}))
        torch.cuda.synchronize(dev)
        log["denoising"]["post"] = mem()
        log["peak_memory"] = max(log["peak_memory"], log["denoising"]["post"]["peak_memory"])
        log["denoising"]["time"] = round(time.time() - t0, 3)
        log["denoising"]["iter_time"] = iter_time
        log["denoising"].update(self.last_sampler)
        if block_cache is not None:
            log["denoising"]["block_cache"] = self.last_block_cache
        if any(self.last_guidance[k] != v for k, v in _DEFAULT_GUIDANCE.items()):  # (a key only when an option is set)
            log["denoising"]["guidance"] = self.last_guidance
        if reference_image_path is not None:
            log["denoising"]["reference"] = self.last_reference
        if condition_image_path is not None:
            log["denoising"]["condition"] = self.last_condition
        if self.last_skip_layer_guidance is not None:
            log["denoising"]["skip_layer_guidance"] = self.last_skip_layer_guidance
        if self.last_perturbed_attention_guidance is not None:
            log["denoising"]["perturbed_attention_guidance"] = self.last_perturbed_attention_guidance
        if self.last_controlnet is not None:
            log["denoising"]["controlnet"] = self.last_controlnet
        if self.last_ip_adapter is not None:
            log["denoising"]["ip_adapter"] = self.last_ip_adapter
        if self.last_edit is not None:
            log["denoising"]["edit"] = self.last_edit

        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.time()
        log["decoding"]["pre"] = mem()
        _, u8, _ = self.decoder.decode(latents)
        if mask_path is not None and composite:
            u8 = self.composite_image(u8, image_path, mask_path)
        elif condition_mask_path is not None and composite:  # (fill: the kept pixels of the condition image, at the size they came in)
            from . import ops
            px, masks = self._condition_pixels
            u8 = ops.image_composite(u8.contiguous(), torch.from_numpy(px).to(u8.device), torch.from_numpy(masks).to(u8.device))
        torch.cuda.synchronize(dev)
        log["decoding"]["post"] = mem()
        log["peak_memory"] = max(log["peak_memory"], log["decoding"]["post"]["peak_memory"])
        log["decoding"]["time"] = round(time.time() - t0, 3)

        if verbose:
            logger.info("============= Summary =============")
            logger.info(f"Text encoder: {log['text_encoding']['time']:.1f}s")
            logger.info(f"Denoising: {log['denoising']['time']:.1f}s")
            logger.info(f"Image decoder: {log['decoding']['time']:.1f}s")
            logger.info(f"Peak memory: {log['peak_memory']:.1f}GB")

        # reference: mx.concatenate(decoded, axis=0) stacks a batch vertically (:525)
        x = u8.reshape(-1, u8.shape[2], 3).cpu().numpy()
        log["total_time"] = round(time.time() - start_time, 3)
        from PIL import Image
        return Image.fromarray(x), log

    # -- helpers (same names as the reference) ----------------------------------------------
    def get_noise(self, seed, x_T):
        """mlx/__init__.py:553-557: numpy global RNG, drawn NCHW, returned NHWC (float32)."""
        np.random.seed(seed)
        noise = np.random.randn(*x_T.transpose(0, 3, 1, 2).shape)
        return noise.astype(np.float32).transpose(0, 2, 3, 1)

    def get_sigmas(self, sampler, num_steps: int):
        return get_sigmas(sampler, num_steps)

    def read_image(self, image_path):
        """mlx/__init__.py:536-551: RGB in [-1, 1], NHWC float32 [1,H,W,3]; sizes are cut down to a
        multiple of 64 with a LANCZOS resize.  ``image_path`` may also be a PIL image or an HWC uint8 array."""
        arr = (read_image_u8(image_path).astype(np.float32) / 255) * 2 - 1.0
        return torch.from_numpy(np.ascontiguousarray(arr[None])).to(self.device)

    def composite_image(self, u8: Tensor, image, mask) -> Tensor:
        """Inpainting paste-back (no reference counterpart): ``u8`` = decoded images uint8 [B, H, W, 3] on the GPU (``decoder.decode`` /
        ``decode_async``), ``image`` / ``mask`` as ``generate_image`` takes them -> uint8 [B, H, W, 3] with the input image's bytes where the
        mask is 0, the decoder's where it is 255 and the rounded blend between."""
        from . import ops
        orig = read_image_u8(image)
        if orig.shape != tuple(u8.shape[1:]):
            raise ValueError(f"the image is {orig.shape[0]}x{orig.shape[1]} after read_image, the decoded images {u8.shape[1]}x{u8.shape[2]}")
        masks = _read_masks(mask, orig.shape[:2], u8.shape[0])
        return ops.image_composite(u8.contiguous(), torch.from_numpy(np.ascontiguousarray(orig)).to(u8.device),
                                   torch.from_numpy(masks).to(u8.device))

    def encode_image_to_latents(self, image_path, seed):
        """mlx/__init__.py:586-594: mean + std * noise of the VAE posterior, NHWC float32 on the device."""
        self.load_vae_encoder()
        image = self.read_image(image_path)
        moments = self.encoder.encode(image)
        b, h, w, _ = moments.shape
        mean_like = np.empty((b, h, w, self.vae_encoder_config.out_channels // 2), dtype=np.float32)
        noise = torch.from_numpy(self.get_noise(seed, mean_like)).to(self.device)
        return self.encoder.sample(moments, noise)

    def condition_tokens(self, images: np.ndarray, masks: Optional[np.ndarray]) -> Tensor:
        """``read_condition_images``' arrays -> the condition token rows bf16 [1 or n, S_i, condition_features] on the device (published FLUX sampling
        code: prepare_fill / prepare_control, with the posterior's mean in place of a sample).  No masks: the control layout."""
        from . import ops
        if masks is None:
            image = torch.from_numpy((images.astype(np.float32) / 255) * 2 - 1.0).to(self.device)
            return ops.fill_condition_tokens(self.latent_format.process_in(self.encode_mean_latents(image)), None, self.mmdit_config.patch_size)
        n = max(images.shape[0], masks.shape[0])
        px = torch.from_numpy(np.array(np.broadcast_to(images, (n, *images.shape[1:])))).to(self.device)  # (a copy: one image for several masks)
        m = torch.from_numpy(masks).to(self.device)
        z = self.latent_format.process_in(self.encode_mean_latents(ops.image_mask_out(px, m)))
        return ops.fill_condition_tokens(z, m, self.mmdit_config.patch_size)

    def encode_reference_to_latents(self, refs: np.ndarray) -> Tensor:
        """Reference images uint8 [n, H, W, 3] (``_read_references``) -> the MEAN of the VAE posterior, NHWC float32 [n, H/8, W/8, L] on the device:
        the encoder's ``sample`` with a zero noise tensor, so the same reference gives the same conditioning whatever the seed."""
        return self.encode_mean_latents(torch.from_numpy((refs.astype(np.float32) / 255) * 2 - 1.0).to(self.device))

    def encode_mean_latents(self, image: Tensor) -> Tensor:
        """``image``: f32 [n, H, W, 3] in [-1, 1] on the device -> the MEAN of the VAE posterior, NHWC float32 [n, H/8, W/8, L]"""
        self.load_vae_encoder()
        moments = self.encoder.encode(image)
        b, h, w, _ = moments.shape
        zeros = torch.zeros(b, h, w, self.vae_encoder_config.out_channels // 2, dtype=torch.float32, device=self.device)
        return self.encoder.sample(moments, zeros)

    def get_empty_latent(self, *shape):
        return np.ones([1, *shape, 16], dtype=np.float32) * np.float32(0.0609)

    def max_denoise(self, sigmas):
        return max_denoise(self.sampler, sigmas)

    def decode_latents_to_image(self, x_t):
        """mlx/__init__.py:581-584: float image in [0,1], NHWC."""
        img, _, _ = self.decoder.decode(x_t)
        return img

    def decode_async(self, latents: Tensor) -> "PendingDecode":
        """Serving helper with no reference counterpart (the reference decodes inline, mlx/__init__.py:497-530): enqueue the VAE
        decode of ``latents`` on the pipeline's side stream, behind an event on the current stream, and return at once -- the
        denoising of the NEXT image then overlaps this one's decode (the decoder's GroupNorm passes and 128-channel convs are
        HBM-bound, the MMDiT GEMMs MFMA-bound).  ``PendingDecode.result()`` hands back (image_f32, image_u8) once the current
        stream has been made to wait for the decode.  Same kernels, same results as ``decoder.decode``.

        Memory: the side stream owns a SECOND decoder workspace (the weights are shared): about 1.5 GB at 1024 x 1024 for one
        image, over 10 GB for eight, held from the first call until ``release_async_decoder()`` (or the pipeline) drops it."""
        if not hasattr(self, "_decode_stream"):
            self._decode_stream = torch.cuda.Stream(device=self.device)
            # the side stream owns a decoder engine of its own (same weight tensors, its own workspace and split flags): an inline
            # ``decoder.decode`` on the caller's stream may run while a PendingDecode is in flight without sharing scratch with it;
            # consecutive async decodes are ordered by the side stream itself
            from .engine import VAEDecoderEngine
            self._async_decoder = VAEDecoderEngine(self.decoder.config, self.decoder.weights)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self._decode_stream):
            self._decode_stream.wait_event(ready)
            latents.record_stream(self._decode_stream)
            img, u8, _ = self._async_decoder.decode(latents)
            done = torch.cuda.Event()
            done.record(self._decode_stream)
        return PendingDecode(img, u8, done, self.device)

    def release_async_decoder(self) -> None:
        """Drop the side stream's decoder engine and its workspace (``decode_async`` builds them again on its next call).  Waits for
        the side stream first, so that no decode in flight loses its scratch."""
        if hasattr(self, "_decode_stream"):
            self._decode_stream.synchronize()
            del self._async_decoder
            del self._decode_stream
            torch.cuda.empty_cache()


class PendingDecode:
    """A VAE decode in flight on the pipeline's side stream (DiffusionPipeline.decode_async)."""

    def __init__(self, img, u8, done, device):
        self._img, self._u8, self._done, self._device = img, u8, done, device

    def result(self):
        cur = torch.cuda.current_stream(self._device)
        cur.wait_event(self._done)
        # the tensors were allocated under the side stream: tell the caching allocator that the caller's stream reads them, so
        # that their blocks are not handed to the next side-stream decode while those readers are still queued
        self._img.record_stream(cur)
        self._u8.record_stream(cur)
        return self._img, self._u8


class FluxPipeline(DiffusionPipeline):
    _IS_FLUX = True

    def __init__(
        self,
        w16: bool = False,
        shift: float = 1.0,
        use_t5: bool = True,
        model_version: str = "argmaxinc/mlx-FLUX.1-schnell",
        low_memory_mode: bool = True,
        a16: bool = False,
        local_ckpt=None,
        quantize_mmdit: bool = False,
        **kw,
    ):
        self.quantize_mmdit = quantize_mmdit
        super().__init__(w16=w16, shift=shift, use_t5=True, model_version=model_version,
                         low_memory_mode=low_memory_mode, a16=a16, local_ckpt=local_ckpt, **kw)

    def _init_sampler(self, shift):
        self.sampler = FluxSampler(shift=shift)
        self.latent_format = FluxLatentFormat()
        self.use_t5 = True
        self.use_clip_g = False

    def encode_text(self, text: str, cfg_weight: float = 7.5, negative_text: str = ""):
        """mlx/__init__.py:642-671: FLUX ignores the negative prompt, batch 1."""
        if self._text_encoder is not None:
            return self._text_encoder(text, cfg_weight, negative_text)
        return self._synthetic_conditioning(text, 1)


class CFGDenoiser:
    """mlx/__init__.py:674-719"""

    def __init__(self, model: DiffusionPipeline):
        self.model = model
        self._timesteps: List[float] = []
        self.block_cache_record = None  # what sample_euler decided per step under extra_args["block_cache"]
        self.guidance_record = None  # what sample_steps ran under extra_args["guidance"]
        self.skip_layer_record = None  # what sample_steps ran under extra_args["skip_layer_guidance"]
        self.perturbed_attention_record = None  # ... under extra_args["perturbed_attention_guidance"]
        self.controlnet_record = None  # ... under extra_args["controlnet"]

    def cache_modulation_params(self, pooled_text_embeddings, timesteps):
        self._timesteps = [float(t) for t in timesteps]
        self.model.mmdit.cache_modulation_params(pooled_text_embeddings, self._timesteps)

    def clear_cache(self):
        # the reference re-reads the adaLN weights from disk here (:686-689); they stay resident
        # in HBM in this build, so there is nothing to do.
        pass

    def step_index(self, timestep: float) -> int:
        return self._timesteps.index(float(timestep))  # first match, like the reference's dict key (Q11)

    def __call__(self, x_t, timestep, sigma, conditioning, cfg_weight: float = 7.5, pooled_conditioning=None):
        """Returns the (CFG-combined) x0 prediction, fp32, same shape as x_t."""
        from . import ops
        mm, cfg = self.model.mmdit, self.model.mmdit_config
        cfg_on = cfg_weight > 0
        tok = mm.patchify(x_t.contiguous(), dup=2 if cfg_on else 1)
        if mm.dtype == torch.float16:  # (bf16 -> fp16 of the encoders' output: exact in range)
            conditioning = conditioning.to(torch.float16).contiguous()
        out = mm.forward_tokens(tok, conditioning, self.step_index(timestep))
        den = x_t.clone()
        ops.euler_cfg_step(den, out, tok, den.shape[0], cfg_on, cfg.patch_size, int(cfg.patchify_via_reshape), float(sigma), 0.0,
                           float(cfg_weight))  # x + d*(0 - sigma) = x0
        return den


def append_dims(x, target_dims):
    """mlx/__init__.py:750-753"""
    dims_to_append = target_dims - x.ndim
    return x[(...,) + (None,) * dims_to_append]


def to_d(x, sigma, denoised):
    """mlx/__init__.py:756-758"""
    return (x - denoised) / sigma


def _tile_conditioning(conditioning: Tensor, pooled: Tensor, n_img: int, cfg_on: bool, is_flux: bool):
    """Conditioning rows -> the engine's batch layout for ``n_img`` images denoised in one step loop (a seed list):
    CFG on: [prompt x n_img, negative x n_img] (the layout dk_euler_cfg_step pairs up); CFG off: one prompt row per image.
    Accepted inputs: the reference's rows ([prompt, negative] from encode_text for SD3, mlx/__init__.py:197-251; one row for
    FLUX, :642-671), tiled here per image, or rows the caller already laid out per image (n_img, or 2 * n_img with CFG).
    SD3 with CFG off keeps the prompt row (the reference cannot run that case)."""
    n = conditioning.shape[0]
    if pooled.shape[0] != n:
        raise ValueError(f"conditioning has {n} rows, pooled conditioning {pooled.shape[0]}")

    def rep(t, rows):
        return torch.cat([t[r:r + 1].expand(n_img, *t.shape[1:]) for r in rows], 0)

    if cfg_on:
        if n == 2 * n_img and (n_img > 1 or n == 2):
            return conditioning, pooled  # [prompt, negative] for one image, or laid out per image by the caller
        if n == 2:
            return rep(conditioning, (0, 1)), rep(pooled, (0, 1))
        return conditioning, pooled  # mismatch: reported by the caller
    if n == 2 and not is_flux:  # encode_text's [prompt, negative]: the negative row is unused without guidance
        return rep(conditioning, (0,)), rep(pooled, (0,))
    if n == 1 and n_img > 1:
        return rep(conditioning, (0,)), rep(pooled, (0,))
    return conditioning, pooled


_HEUN_BLOCK_CACHE = ("sampler 'heun' cannot run together with block_cache: its two model evaluations per step do not map onto the policy's "
                     "decide(step, n_steps, rel); a policy for two-evaluation steps is out of scope -- use sampler 'ab2' (one evaluation per step)")


_DEFAULT_GUIDANCE = {"mode": "cfg", "guidance_rescale": 0.7, "apg_eta": 0.0, "apg_norm_threshold": 0.0, "apg_momentum": 0.0, "interval": None}


def _guidance_options(guidance, rescale, eta, norm_threshold, momentum, interval, cfg_weight):
    """The guidance keywords of ``denoise_latents`` -> None when they are all at their defaults (the loops run as they always did), else the dict
    ``sample_steps`` takes as ``extra_args["guidance"]``.  Refused: an unknown mode, a parameter that is not finite, a rescale factor outside
    [0, 1], an interval that is not lo <= hi, and any non-default option without classifier-free guidance (``cfg_weight <= 0``: FLUX)."""
    opts = {"mode": check_guidance(guidance), "guidance_rescale": float(rescale), "apg_eta": float(eta), "apg_norm_threshold": float(norm_threshold),
            "apg_momentum": float(momentum), "interval": None if interval is None else check_interval(interval)}
    for k in ("guidance_rescale", "apg_eta", "apg_norm_threshold", "apg_momentum"):
        if not np.isfinite(opts[k]):
            raise ValueError(f"{k} must be finite, got {opts[k]}")
    if not 0.0 <= opts["guidance_rescale"] <= 1.0:
        raise ValueError(f"guidance_rescale must lie in [0, 1], got {opts['guidance_rescale']}")
    if opts == _DEFAULT_GUIDANCE:
        return None
    if not cfg_weight > 0:
        raise ValueError("the guidance options (guidance, guidance_rescale, apg_*, guidance_interval) need classifier-free guidance: cfg_weight is "
                         f"{cfg_weight}, so there is no negative prediction to combine (FLUX runs without one)")
    return opts


def _skip_layer_options(scale, layers, interval, model_version, mmdit_config, is_flux, cfg_weight, block_cache):
    """The skip-layer keywords of ``denoise_latents`` -> None when the feature is off (``scale`` None, the loops run as they always did), else the dict
    ``sample_steps`` takes as ``extra_args["skip_layer_guidance"]``: {"scale", "layers", "interval"}.  What the caller leaves None comes from the
    model version's published recipe (``config.SKIP_LAYER_GUIDANCE``); ``scale`` True asks for its scale as well.  Refused: layers or an interval
    without a scale, FLUX, ``cfg_weight <= 0``, ``block_cache``, a version without a recipe that names no layers, and whatever
    ``sampler.check_skip_layer_guidance`` refuses."""
    if scale is None:
        if layers is not None or interval is not None:
            raise ValueError("skip_layers / skip_layer_interval need skip_layer_guidance (the scale of the term; None is off)")
        return None
    if is_flux:
        raise ValueError("skip-layer guidance is the SD3 family's: FLUX runs without classifier-free guidance and its single blocks have no skip form")
    if not cfg_weight > 0:
        raise ValueError(f"skip-layer guidance needs classifier-free guidance: cfg_weight is {cfg_weight}, so there is no guided prediction to add to")
    if block_cache is not None:
        raise ValueError("skip-layer guidance cannot run together with block_cache: there is no cache policy for a forked row group yet")
    recipe = SKIP_LAYER_GUIDANCE.get(model_version, {})
    if scale is True:
        if "scale" not in recipe:
            raise ValueError(f"skip_layer_guidance=True takes the scale published with the model version, and {model_version} has none: name a scale")
        scale = recipe["scale"]
    if layers is None:
        if "layers" not in recipe:
            raise ValueError(f"no skip layers are published for {model_version}: name them (skip_layers=...)")
        layers = recipe["layers"]
    if interval is None:
        interval = recipe.get("interval")
    scale, layers, interval = check_skip_layer_guidance(scale, layers, interval, mmdit_config.depth_multimodal)
    return {"scale": scale, "layers": layers, "interval": interval}


def _perturbed_attention_options(scale, layers, interval, mmdit_config, is_flux, cfg_weight, block_cache, reference, condition, slg):
    """The perturbed-attention keywords of ``denoise_latents`` -> None when the feature is off (all None), else the dict ``sample_steps`` takes as
    ``extra_args["perturbed_attention_guidance"]``: {"scale", "layers", "interval"} (interval None: every guided row).  There is no published recipe:
    a scale without layers and layers (or an interval) without a scale are refused, and so are FLUX, ``cfg_weight <= 0``, ``block_cache``, an fp8
    engine, a reference image, a condition, skip-layer guidance in the same call, and whatever ``sampler.check_perturbed_attention_guidance``
    refuses."""
    if scale is None and layers is None and interval is None:
        return None
    if scale is None:
        raise ValueError("pag_layers / pag_interval need pag_scale (the scale of the term; None is off)")
    if layers is None:
        raise ValueError("pag_scale needs pag_layers: no layers are published for perturbed-attention guidance, name them")
    if is_flux:
        raise ValueError("perturbed-attention guidance is the SD3 family's: FLUX runs without classifier-free guidance and its blocks have no perturbed form")
    if not cfg_weight > 0:
        raise ValueError(f"perturbed-attention guidance needs classifier-free guidance: cfg_weight is {cfg_weight}, and the step entry combines both "
                         "CFG rows (PAG without CFG is not built)")
    if block_cache is not None:
        raise ValueError("perturbed-attention guidance cannot run together with block_cache: there is no cache policy for a forked row group yet")
    if mmdit_config.weight_dtype == "fp8_e4m3":
        raise ValueError("perturbed-attention guidance cannot run on an fp8 engine: the identity attention has no MX-fp8 output copy")
    if reference is not None:
        raise ValueError("perturbed-attention guidance cannot run with a reference image: the forked row group has no reference grid")
    if condition is not None:
        raise ValueError("perturbed-attention guidance cannot run with a condition: the forked row group has no condition width")
    if slg is not None:
        raise ValueError("perturbed-attention guidance cannot run together with skip-layer guidance: the engine forks one row group")
    scale, layers, interval = check_perturbed_attention_guidance(scale, layers, interval, mmdit_config.depth_multimodal)
    return {"scale": scale, "layers": layers, "interval": interval}


def controlnet_step_active(i: int, n: int, interval) -> bool:
    """whether step ``i`` of ``n`` runs with the ControlNet under ``interval`` = (start, stop) fractions of the schedule: diffusers'
    control_guidance_start / _end rule, i / n >= start and (i + 1) / n <= stop.  None: every step"""
    if interval is None:
        return True
    start, stop = interval
    return i / n >= start and (i + 1) / n <= stop


def _check_flux_controlnet_config(pipe, controlnet_config) -> None:
    """``controlnet_ckpt`` on a FLUX-family pipeline (``DiffusionPipeline._check_controlnet_config``): the configuration is required and must be a
    FLUX ControlNet's that fits the model; sets ``pipe.controlnet_config``.  Needs no GPU."""
    from .config import validate_control_net_flux
    cfg = pipe.mmdit_config
    if controlnet_config is None:
        raise ValueError("controlnet_ckpt without a controlnet_config is the SD3 family's preset (config.SD3_CONTROLNET_6, diffusers' SD3ControlNetModel): a "
                         "FLUX pipeline names its ControlNet's depths, controlnet_config=config.flux_controlnet_config(n_double, n_single) -- FLUX "
                         "ControlNets (diffusers' FluxControlNetModel) have no canonical depth")
    if cfg.weight_dtype == "fp8_e4m3":
        raise ValueError("controlnet_ckpt cannot be combined with an fp8 engine: the fp8 LayerNorm kernels take no tap")
    if cfg.condition_features != 0 or getattr(pipe, "condition", None) is not None:
        raise ValueError("controlnet_ckpt cannot be combined with condition= (FLUX.1 Fill / Canny / Depth): the engine carries one kind of image "
                         "conditioning at a time")
    if not getattr(controlnet_config, "control_net_flux", False):
        raise ValueError("controlnet_config must be a FLUX control-net configuration (control_net_flux=True, config.flux_controlnet_config(n_double, "
                         "n_single)); control_net=True is the SD3 family's")
    ccfg = controlnet_config
    validate_control_net_flux(ccfg)
    if (ccfg.hidden_size != cfg.hidden_size or ccfg.num_heads != cfg.num_heads or ccfg.patch_dim != cfg.patch_dim
            or ccfg.depth_multimodal > cfg.depth_multimodal or ccfg.depth_unified > cfg.depth_unified):
        raise ValueError(f"the ControlNet (hidden {ccfg.hidden_size}, {ccfg.num_heads} heads, patch_dim {ccfg.patch_dim}, ({ccfg.depth_multimodal}, "
                         f"{ccfg.depth_unified}) blocks) does not fit the model (hidden {cfg.hidden_size}, {cfg.num_heads} heads, patch_dim "
                         f"{cfg.patch_dim}, ({cfg.depth_multimodal}, {cfg.depth_unified}) blocks): the taps are added to its stream")
    pipe.controlnet_config = ccfg


def _check_ip_adapter_config(pipe, ip_config, controlnet_ckpt) -> None:
    """``ip_adapter_ckpt`` on a pipeline: the FLUX family's, one kind of added conditioning at a time; sets ``pipe.ip_adapter_config``.  Needs no GPU."""
    from .config import FLUX_IP_ADAPTER, IPAdapterConfig, validate_ip_adapter
    cfg = pipe.mmdit_config
    if not pipe._IS_FLUX:
        raise ValueError("ip_adapter_ckpt is the FLUX family's (FluxPipeline): SD3 and SD3.5 IP-Adapters are not built")
    if cfg.weight_dtype == "fp8_e4m3":
        raise ValueError("ip_adapter_ckpt cannot be combined with an fp8 engine: the fp8 LayerNorm kernels take no tap")
    if getattr(pipe, "condition", None) is not None:
        raise ValueError("ip_adapter_ckpt cannot be combined with condition= (FLUX.1 Fill / Canny / Depth): the engine refuses a condition width beside "
                         "the adapter")
    if controlnet_ckpt is not None:
        raise ValueError("ip_adapter_ckpt cannot be combined with controlnet_ckpt: the LayerNorm launch has one tap operand")
    ipc = FLUX_IP_ADAPTER if ip_config is None else ip_config
    if not isinstance(ipc, IPAdapterConfig):
        raise ValueError(f"ip_adapter_config must be a config.IPAdapterConfig, got {type(ipc).__name__}")
    validate_ip_adapter(cfg, ipc)
    pipe.ip_adapter_config = ipc


def _ip_adapter_options(pipe, embeds, scale, n_img, cfg_weight, block_cache, reference):
    """The IP-Adapter keywords of one call -> None (a pipeline without an adapter and no keyword) or {"embeds": f32 [1 or n_img, E], "scale"}.
    Refused, each naming its rule: the keywords on a pipeline built without an adapter and their absence on one built with it, ``cfg_weight > 0``,
    ``block_cache``, a reference image, embeddings of another width or count."""
    ipc = getattr(pipe, "ip_adapter_config", None)
    if ipc is None:
        if embeds is not None or float(scale) != 1.0:
            raise ValueError("ip_adapter_image_embeds / ip_adapter_scale need a pipeline built with an IP-Adapter (ip_adapter_ckpt=)")
        return None
    if embeds is None:
        raise ValueError("a pipeline built with an IP-Adapter needs ip_adapter_image_embeds in every call (ip_adapter_scale=0 switches it off)")
    if cfg_weight > 0:
        raise ValueError("an IP-Adapter cannot run with cfg_weight > 0: negative image embeds (true CFG) are not built")
    if block_cache is not None:
        raise ValueError("an IP-Adapter cannot run together with block_cache: the engine refuses the block cache beside the adapter")
    if reference is not None:
        raise ValueError("an IP-Adapter cannot run together with reference_image_path: the engine refuses a reference grid beside the adapter")
    scale = float(scale)
    if not np.isfinite(scale):
        raise ValueError(f"ip_adapter_scale must be finite, got {scale}")
    rows = [embeds] if not isinstance(embeds, (list, tuple)) else list(embeds)
    rows = [np.asarray(r.detach().float().cpu() if isinstance(r, torch.Tensor) else r, dtype=np.float32) for r in rows]
    e = np.concatenate([r.reshape(1, -1) if r.ndim == 1 else r for r in rows], axis=0)
    if e.ndim != 2 or e.shape[1] != ipc.embed_dim:
        raise ValueError(f"ip_adapter_image_embeds must be [E], [n, E] or a list of [E] with E = {ipc.embed_dim}, got {tuple(e.shape)}")
    if e.shape[0] not in (1, n_img):
        raise ValueError(f"{e.shape[0]} image embeddings for {n_img} seeds: one for all, or one per seed (several image prompts at once are not built)")
    if not np.isfinite(e).all():
        raise ValueError("ip_adapter_image_embeds must be finite")
    return {"embeds": np.ascontiguousarray(e), "scale": scale}


def _cache_ip_adapter(mm, ip: Optional[dict], now: int, n_img: int) -> None:
    """Behind ``_prepare_rows``: the image prompt's keys and values cached for those rows, shared or per image like ``_cache_reference``, and the scale"""
    if ip is None:
        return
    tok = ip["tokens"]
    if tok.shape[0] == 1:
        mm.cache_ip_tokens(tok, per_image=False)
    else:
        mm.cache_ip_tokens(tok.repeat(now // n_img, 1, 1).contiguous(), per_image=True)
    mm.set_ip_scale(ip["scale"])


def _controlnet_options(pipe, image, scale, interval, n_img, out_hw, block_cache, slg, pag, reference=None, condition=None):
    """The ControlNet keywords of one call -> None (a pipeline without a ControlNet and no keyword) or {"pixels": uint8 [1 or n_img, H, W, 3],
    "scale", "interval"}.  Refused, each naming its rule: the keywords on a pipeline built without a ControlNet and their absence on one built
    with it, ``block_cache``, skip-layer and perturbed-attention guidance, a reference image or a condition (the FLUX family's: the engine
    refuses taps beside either), a control image of another size than the output."""
    has = getattr(pipe, "controlnet", None) is not None
    if not has:
        if image is not None or interval is not None or float(scale) != 1.0:
            raise ValueError("controlnet_image_path / controlnet_scale / controlnet_interval need a pipeline built with a ControlNet (controlnet_ckpt=)")
        return None
    if image is None:
        raise ValueError("a pipeline built with a ControlNet needs controlnet_image_path in every call: the ControlNet was trained to see a control image")
    if reference is not None:
        raise ValueError("a ControlNet cannot run together with reference_image_path: the reference rows of the stream would need taps of their own")
    if condition is not None:
        raise ValueError("a ControlNet cannot run together with a condition (condition_image_path): the engine carries one kind of image conditioning at a time")
    if block_cache is not None:
        raise ValueError("a ControlNet cannot run together with block_cache: the cached effect of blocks 1 .. L-1 would hold another step's taps")
    if slg is not None or pag is not None:
        raise ValueError("a ControlNet cannot run together with skip-layer or perturbed-attention guidance: the forked row group would need taps of its own")
    scale = float(scale)
    if not np.isfinite(scale):
        raise ValueError(f"controlnet_scale must be finite, got {scale}")
    if interval is not None:
        interval = tuple(float(v) for v in interval)
        if len(interval) != 2 or not all(np.isfinite(v) for v in interval):
            raise ValueError(f"controlnet_interval must be (start, stop), two finite fractions of the schedule, got {interval}")
    px = _read_references(image, n_img)  # (a path, a PIL image or an array, or one per seed; sides that are multiples of 16; never resized)
    if tuple(px.shape[1:3]) != tuple(out_hw):
        raise ValueError(f"the control image is {px.shape[1]}x{px.shape[2]}, the output {out_hw[0]}x{out_hw[1]}: it must have the output's size "
                         "(it is not resized here)")
    return {"pixels": px, "scale": scale, "interval": interval}


def _prepare_control(lp_control: Optional[dict], now: int, n_img: int, latent_hw, conditioning: Tensor, pooled: Tensor, timesteps) -> None:
    """Behind ``_prepare_rows``: the ControlNet engine prepared for the same rows as the main engine, with its own modulation table, context and
    control-image share, and a taps tensor of that shape"""
    if lp_control is None:
        return
    cn, tok = lp_control["engine"], lp_control["tokens"]
    cn.prepare(now, latent_hw, conditioning.shape[1], len(timesteps))
    cn.cache_modulation_params(pooled, [float(t) for t in timesteps])
    cn.cache_context(conditioning)
    if tok.shape[0] == 1:
        cn.cache_control_image(tok, per_image=False)
    else:
        cn.cache_control_image(tok.repeat(now // n_img, 1, 1).contiguous(), per_image=True)
    lp_control["taps"] = torch.empty(cn.taps_shape(), dtype=cn.dtype, device=tok.device)


class _Loop(NamedTuple):
    """what a step loop works on once the engine is prepared (``_loop_setup``)"""
    pipe: object
    mm: object
    sigmas: np.ndarray
    cfg_weight: float
    cfg_on: bool
    n_img: int
    policy: object
    x: Tensor
    mask: Optional[Tensor]
    x_orig: Optional[Tensor]
    noise: Optional[Tensor]
    tok: Tensor
    out: Tensor
    conditioning: Tensor
    pooled: Tensor
    timesteps: object
    reference: Optional[Tensor] = None  # the reference latent f32 [1 or n_img, rh, rw, C] behind ``extra_args["reference"]``, or None
    condition: Optional[Tensor] = None  # the condition token rows bf16 [1 or n_img, S_i, condition_features] behind ``extra_args["condition"]``, or None
    slg: Optional[dict] = None  # ``extra_args["skip_layer_guidance"]`` (``_skip_layer_options``), or None
    pag: Optional[dict] = None  # ``extra_args["perturbed_attention_guidance"]`` (``_perturbed_attention_options``), or None: never both
    # ``extra_args["controlnet"]``: {"engine": the ControlNet's MMDiTEngine, "tokens": the control image's tokens [1 or n_img, S_i, p*p*C], "scale",
    # "interval"} plus "taps", the tensor ``_prepare_control`` allocates for the rows the engines hold; or None
    control: Optional[dict] = None
    ip: Optional[dict] = None  # ``extra_args["ip_adapter"]``: {"tokens": the image prompt's tokens bf16 [1 or n_img, N, C], "scale"}, or None

    @property
    def forked(self) -> Optional[dict]:
        """the options of the feature that forks a third row group, skip-layer or perturbed-attention guidance: {"scale", "layers", ...}, or None"""
        return self.slg if self.slg is not None else self.pag

    def set_fork(self, on: bool) -> None:
        """the engine's setter of that feature: its layers on ``n_img`` fork rows, or off"""
        setter = self.mm.set_skip_layers if self.slg is not None else self.mm.set_perturbed_attention
        setter(self.forked["layers"] if on else None, self.n_img if on else 0)


def _cache_condition(mm, condition: Optional[Tensor], now: int, n_img: int) -> None:
    """Behind ``_prepare_rows``: the condition's share of x_embedder computed once for those rows, shared or per image like ``_cache_reference``"""
    if condition is None:
        return
    if condition.shape[0] == 1:
        mm.cache_condition(condition, per_image=False)
    else:
        mm.cache_condition(condition.repeat(now // n_img, 1, 1).contiguous(), per_image=True)


def _prepare_rows(mm, now: int, latent_hw, text_len: int, n_t: int, reference: Optional[Tensor]) -> None:
    """``MMDiTEngine.prepare`` for ``now`` batch rows, with the reference latent's grid when there is one (none: the engine's grid is turned off)"""
    if reference is None:
        mm.prepare(now, latent_hw, text_len, n_t)  # (the call as it always was)
    else:
        mm.prepare(now, latent_hw, text_len, n_t, reference_size=tuple(reference.shape[1:3]))


def _cache_reference(mm, reference: Optional[Tensor], now: int, n_img: int) -> None:
    """Behind ``_prepare_rows``: the reference embedded once for those rows: one shared reference is broadcast, per-image ones follow the engine's
    batch layout ([prompt x n_img, negative x n_img] with CFG)."""
    if reference is None:
        return
    if reference.shape[0] == 1:
        mm.cache_reference(reference, per_image=False)
    else:
        tok = mm.patchify(reference.to(torch.float32).contiguous())
        mm.cache_reference(tok.repeat(now // n_img, 1, 1).contiguous(), per_image=True)


def _loop_setup(model: "CFGDenoiser", x: Tensor, sigmas, extra_args, guided: bool = True) -> _Loop:
    """The part of a step loop in front of its first step: conditioning rows in the engine's batch layout, timesteps, the engine prepared with its
    modulation table and cached context, the fp32 copy of the latent, the inpainting operands and the first patchified tokens.
    ``guided`` False (a guidance interval that leaves out the first evaluation): the engine starts on the prompt rows alone, ``_set_rows``'s state."""
    extra_args = {} if extra_args is None else dict(extra_args)
    pipe = model.model
    mm = pipe.mmdit
    sigmas = np.asarray(sigmas, dtype=np.float32)
    cfg_weight = float(extra_args.get("cfg_weight", 7.5))
    cfg_on = cfg_weight > 0
    conditioning = extra_args["conditioning"]
    pooled = extra_args.pop("pooled_conditioning")
    if conditioning.dim() == 4:
        conditioning = conditioning.squeeze(2)
    n_img = x.shape[0]
    rows = n_img * (2 if cfg_on else 1)
    conditioning, pooled = _tile_conditioning(conditioning, pooled, n_img, cfg_on, pipe._IS_FLUX)
    if conditioning.shape[0] != rows or pooled.shape[0] != rows:
        raise ValueError(f"conditioning batch {conditioning.shape[0]} does not match latent batch {rows}")
    # (an fp16 engine: the bf16 -> fp16 cast of the encoders' output is exact in range)
    conditioning = conditioning.to(pipe.device, mm.dtype).contiguous()
    pooled = pooled.to(pipe.device, mm.dtype).contiguous()

    # model timesteps are sigma*1000 rounded to the reference pipeline's activation dtype (quirk Q1): fp16 for SD3, bf16 for FLUX
    timesteps = _round_to_dtype(pipe.sampler.timestep(sigmas), pipe.timestep_dtype)
    policy = extra_args.get("block_cache")
    if policy is not None and not hasattr(policy, "decide"):
        from .sampler import BlockCachePolicy
        policy = BlockCachePolicy(policy)
    mm.enable_block_cache(policy is not None)  # (off: the engine's workspace and launches are what they are without the feature)
    now = rows if guided else n_img  # ([prompt x n_img, negative x n_img]: the prompt rows come first)
    reference = extra_args.get("reference")
    if reference is not None:
        reference = reference.to(pipe.device, torch.float32).contiguous()
        if reference.dim() != 4 or reference.shape[0] not in (1, n_img) or reference.shape[3] != x.shape[3]:
            raise ValueError(f"the reference latent {tuple(reference.shape)} does not match the latent {tuple(x.shape)}: [1 or n_img, rh, rw, C]")
    _prepare_rows(mm, now, x.shape[1:3], conditioning.shape[1], len(timesteps), reference)
    _cache_reference(mm, reference, now, n_img)
    condition = extra_args.get("condition")
    if condition is not None and (condition.dim() != 3 or condition.shape[0] not in (1, n_img)):
        raise ValueError(f"the condition tokens {tuple(condition.shape)} do not match {n_img} images: [1 or n_img, S_i, condition_features]")
    _cache_condition(mm, condition, now, n_img)
    model.cache_modulation_params(pooled[:now], timesteps)
    mm.cache_context(conditioning[:now])  # context_embedder is step-invariant (the reference recomputes it in every call, mmdit.py:195)
    ip = extra_args.get("ip_adapter")
    if ip is not None and (ip["tokens"].dim() != 3 or ip["tokens"].shape[0] not in (1, n_img)):
        raise ValueError(f"the image-prompt tokens {tuple(ip['tokens'].shape)} do not match {n_img} images: [1 or n_img, N, C]")
    _cache_ip_adapter(mm, ip, now, n_img)
    control = extra_args.get("controlnet")
    if control is not None:
        control = dict(control)
        if policy is not None or extra_args.get("skip_layer_guidance") is not None or extra_args.get("perturbed_attention_guidance") is not None:
            raise ValueError("extra_args['controlnet'] cannot run together with block_cache, skip-layer or perturbed-attention guidance")
        if control["tokens"].dim() != 3 or control["tokens"].shape[0] not in (1, n_img):
            raise ValueError(f"the control tokens {tuple(control['tokens'].shape)} do not match {n_img} images: [1 or n_img, S_i, patch_dim]")
        _prepare_control(control, now, n_img, x.shape[1:3], conditioning[:now], pooled[:now], timesteps)

    x = x.to(torch.float32).contiguous().clone()
    mask = extra_args.get("mask")
    if mask is not None:
        mask, x_orig, noise = (t.to(pipe.device, torch.float32).contiguous() for t in (mask, extra_args["x_orig"], extra_args["noise"]))
        if x_orig.shape != x.shape or noise.shape != x.shape or mask.shape[1:] != x.shape[1:3] or mask.shape[0] not in (1, n_img):
            raise ValueError(f"inpainting operands do not match the latent {tuple(x.shape)}: x_orig {tuple(x_orig.shape)}, "
                             f"noise {tuple(noise.shape)}, mask {tuple(mask.shape)}")
    else:
        x_orig = noise = None
    tok = mm.patchify(x, dup=2 if cfg_on and guided else 1)
    return _Loop(pipe, mm, sigmas, cfg_weight, cfg_on, n_img, policy, x, mask, x_orig, noise, tok, torch.empty_like(tok), conditioning, pooled, timesteps,
                 reference, condition, extra_args.get("skip_layer_guidance"), extra_args.get("perturbed_attention_guidance"), control, ip)


def _set_rows(model: "CFGDenoiser", lp: _Loop, guided: bool, fork: bool = False):
    """The number of row groups changes -- a guidance interval or the window of skip-layer guidance begins or ends: the engine re-prepared for one
    group (the prompt rows alone), two (both CFG rows of every image) or, with ``fork``, three ([prompt x n | negative x n | skip x n], the third a forked
    copy of the first: ``MMDiTEngine.set_skip_layers(layers, n_img)``), its modulation table and context cached again for those rows -- the fork rows
    repeat the prompt's pooled rows; their context and token rows are never read -- and x patchified with the matching ``dup`` -> (tok, out)."""
    live = lp.n_img * (2 if guided else 1)
    now = live + (lp.n_img if fork else 0)
    rows = (lambda t: torch.cat([t[:live], t[:lp.n_img]], 0)) if fork else (lambda t: t[:live])
    _prepare_rows(lp.mm, now, lp.x.shape[1:3], lp.conditioning.shape[1], len(lp.timesteps), lp.reference)
    _cache_reference(lp.mm, lp.reference, now, lp.n_img)
    _cache_condition(lp.mm, lp.condition, now, lp.n_img)
    model.cache_modulation_params(rows(lp.pooled).contiguous(), lp.timesteps)
    lp.mm.cache_context(rows(lp.conditioning).contiguous())
    _cache_ip_adapter(lp.mm, lp.ip, now, lp.n_img)
    if lp.forked is not None:  # (without the options the engine is never told: its calls are what they were)
        lp.set_fork(fork)
    _prepare_control(lp.control, now, lp.n_img, lp.x.shape[1:3], rows(lp.conditioning).contiguous(), rows(lp.pooled).contiguous(), lp.timesteps)
    tok = lp.mm.patchify(lp.x, dup=now // lp.n_img)
    return tok, torch.empty_like(tok)


def _step_loop(model: "CFGDenoiser", lp: _Loop, plan, grows, guide=None, euler: bool = False, srows=None, noise_seeds=None):
    """The host loop behind ``sample_euler`` and ``sample_steps``: per (row, guidance row) one model evaluation -- the engine's head, the policy's
    decision and the chosen tail under the first-block cache -- and one launch of the update, with one device synchronisation per step (the
    reference's mx.eval(x)), which provides iter_time.  ``euler``: the rows are the schedule's Euler rows and the update is dk_euler_cfg_step, the
    reference's statement, instead of the coefficient-row entry.  ``srows`` (``sampler.slg_rows``; None: no row): the evaluations that carry the forked
    third row group and end in dk_slg_cfg_step.  A row with a noise term (``cn != 0``: the stochastic samplers) ends in dk_noisy_cfg_step with the same
    groups instead, the noise drawn in that launch from ``noise_seeds`` (one Python int per image, uploaded once, here).  The operators are looked up on
    ``ops`` at every call."""
    from . import ops
    from .sampler import block_cache_rel
    pipe, mm, _, cfg_weight, cfg_on, n_img, policy, x, mask, x_orig, noise, tok, out = lp[:13]
    pcfg = pipe.mmdit_config
    hist = torch.empty_like(x) if any(r.reads_h or r.writes_h for r in plan) else None  # (never initialised: no row reads it before one wrote it)
    mode = "cfg" if guide is None else guide["mode"]
    beta = 0.0 if guide is None else guide["apg_momentum"]
    gws = mbuf = None
    if mode != "cfg" and any(g.guided for g in grows):  # (the moments' partials and scalars: caller-owned, never initialised)
        gws = torch.empty(ops.guidance_workspace_bytes(*x.shape), dtype=torch.uint8, device=x.device)
    if mode == "apg" and beta != 0.0 and any(g.feeds for g in grows):
        mbuf = torch.empty_like(x)  # (never initialised: the first guided row of a stretch does not read it)
    blend = () if mask is None else (x_orig, noise, mask)
    seeds = None
    if any(r.cn != 0.0 for r in plan):
        if noise_seeds is None or len(noise_seeds) != n_img:
            raise ValueError(f"the plan has rows with a noise term: extra_args['noise_seeds'] must hold one seed per image ({n_img})")
        seeds = ops.seed_tensor(noise_seeds, x.device)
    n_steps = sum(r.ends_step for r in plan)
    record = {"threshold": getattr(policy, "threshold", None), "computed": [], "skipped": [], "rel": []}
    iter_time = []
    step, t0 = 0, None
    on = cfg_on and (grows[0].guided if grows else True)  # whether the engine holds both CFG rows of every image
    fresh = False  # the engine was re-prepared: the first-block cache holds nothing to reuse
    fork = False  # whether it holds the forked third row group of skip-layer guidance
    srows = [False] * len(plan) if srows is None else srows
    control_evals = 0
    for r, g, sl in zip(plan, grows, srows):
        t0 = time.perf_counter() if t0 is None else t0
        if cfg_on and (g.guided != on or sl != fork):
            on, fork = g.guided, sl
            tok, out = _set_rows(model, lp, on, fork) if lp.forked is not None else _set_rows(model, lp, on)
            if policy is not None:
                mm.reset_block_cache()
                fresh = True
        if lp.control is not None:
            # the ControlNet in front of the main forward, on the same stream and the same tokens; a step outside the interval runs without it and
            # with the taps off: the plain launches (Heun's two rows share their step's decision)
            if controlnet_step_active(step, n_steps, lp.control["interval"]):
                lp.control["engine"].control_forward(tok, None, r.index, taps_out=lp.control["taps"])
                if mm.control_taps is None or mm.control_taps[0] is not lp.control["taps"]:
                    cn = lp.control["engine"]
                    if cn.control_net_flux:  # (every tap it writes, its double blocks' first; the main engine maps them onto its own depths)
                        mm.set_flux_control_taps(lp.control["taps"], cn.config.depth_multimodal, lp.control["scale"])
                    else:
                        mm.set_control_taps(lp.control["taps"], lp.control["scale"])
                control_evals += 1
            elif mm.control_taps is not None:
                mm.set_control_taps(None)
        if policy is None:
            mm.forward_tokens(tok, None, r.index, tokens_out=out)
        else:
            rel = block_cache_rel(mm.forward_head(tok, None, r.index).cpu().tolist())  # (.cpu(): the step's synchronisation point)
            skip = bool(policy.decide(step, n_steps, rel)) and not fresh
            fresh = False
            mm.forward_tail(r.index, skip, tokens_out=out)
            record["skipped" if skip else "computed"].append(step)
            record["rel"].append(rel)
        args = (x, out, tok, n_img, on, pcfg.patch_size, int(pcfg.patchify_via_reshape), r.sigma, r.sigma_next, cfg_weight)
        if not euler:
            args += (hist, (r.cx, r.cd, r.ch, r.hx, r.hd), r.reads_h, r.writes_h)
        if r.cn != 0.0:  # (the same groups as the branches below, spelled out as flags)
            group = dict(guided=True, mode=mode, workspace=gws, **({} if guide is None else dict(
                rescale=guide["guidance_rescale"], eta=guide["apg_eta"], norm_threshold=guide["apg_norm_threshold"])), momentum=beta,
                reads_m=mbuf is not None and not g.first, writes_m=mbuf is not None and g.feeds, m=mbuf) if fork or on and mode != "cfg" else {}
            ops.noisy_cfg_step(*args, cn=r.cn, seeds=seeds, draw=r.draw, slg_scale=lp.forked["scale"] if fork else None, **group,
                               **dict(zip(("x_orig", "noise", "mask"), blend)))
        elif fork:
            ops.slg_cfg_step(*args, slg_scale=lp.forked["scale"], mode=mode, workspace=gws, **({} if guide is None else dict(
                rescale=guide["guidance_rescale"], eta=guide["apg_eta"], norm_threshold=guide["apg_norm_threshold"])), momentum=beta,
                reads_m=mbuf is not None and not g.first, writes_m=mbuf is not None and g.feeds, m=mbuf, **dict(zip(("x_orig", "noise", "mask"), blend)))
        elif on and mode != "cfg":
            ops.guided_cfg_step(*args, mode=mode, workspace=gws, rescale=guide["guidance_rescale"], eta=guide["apg_eta"],
                                norm_threshold=guide["apg_norm_threshold"], momentum=beta, reads_m=mbuf is not None and not g.first,
                                writes_m=mbuf is not None and g.feeds, m=mbuf, **dict(zip(("x_orig", "noise", "mask"), blend)))
        else:
            getattr(ops, ("euler" if euler else "lms") + "_cfg_step" + ("_masked" if blend else ""))(*args, *blend)
        if r.ends_step:
            torch.cuda.synchronize(pipe.device)
            iter_time.append(round(time.perf_counter() - t0, 3))
            step, t0 = step + 1, None
    if policy is not None:
        model.block_cache_record = record
    if guide is not None:
        n_g = sum(g.guided for g in grows)
        model.guidance_record = dict(guide, guided_evals=n_g, unguided_evals=len(grows) - n_g)
    if lp.slg is not None:
        model.skip_layer_record = dict(lp.slg, evals=sum(bool(v) for v in srows))
    if lp.pag is not None:
        model.perturbed_attention_record = dict(lp.pag, evals=sum(bool(v) for v in srows))
    if lp.control is not None:
        model.controlnet_record = {"scale": lp.control["scale"], "interval": lp.control["interval"], "evals": control_evals}
    model.clear_cache()
    return x, iter_time


def sample_euler(model: CFGDenoiser, x: Tensor, sigmas, extra_args=None):
    """mlx/__init__.py:761-788.  x: fp32 [n_img,h,w,16] on the GPU (updated copy is returned);
    sigmas: host float32 array.  One device synchronisation per step (the reference's
    mx.eval(x)) provides iter_time.
    Inpainting: ``extra_args["mask"]`` (f32 [1 or n_img, h, w], 1 = repaint) together with ``"x_orig"`` and ``"noise"`` (f32 like x: the
    encoded image after process_in and the draw of the start state) makes every step end in the blend of dk_euler_cfg_step_masked --
    still one launch per step.
    First-block cache: ``extra_args["block_cache"]`` (a float threshold or a policy object, ``sampler.BlockCachePolicy``) turns a step into
    the engine's head, the read of its probe (the step's decision needs it on the host: a synchronisation), and the tail the policy chose;
    the record of the decisions goes to ``model.block_cache_record``."""
    lp = _loop_setup(model, x, sigmas, extra_args)
    plan = step_plan("euler", lp.sigmas)  # (one row per step; its sigma and sigma_next are the schedule's float32 entries)
    try:
        return _step_loop(model, lp, plan, guidance_rows(plan), euler=True)
    finally:
        if lp.control is not None:  # (the main engine's taps are off again when the loop returns or raises)
            lp.mm.set_control_taps(None)


def sample_steps(model: CFGDenoiser, x: Tensor, sigmas, plan, extra_args=None):
    """``sample_euler`` for the second-order samplers (no reference counterpart): ``plan`` = the rows of ``sampler.step_plan(name, sigmas)``, one model
    evaluation each (at the row's entry of the schedule, which is also its row of the cached modulation table -- Heun's corrector reuses the next
    step's), followed by one launch of dk_lms_cfg_step that applies the row's coefficients to x and to the fp32 history buffer allocated here.
    Same operands and ``extra_args`` as ``sample_euler``, inpainting and the first-block cache included: the masked launch blends at the row's
    sigma_next (on Heun's predictor row too, so that the corrector's evaluation sees the re-imposed region), and a plan of one evaluation per
    step (ab2) hands the policy the same step indices as the Euler loop.  A plan with two evaluations in a step (heun) refuses ``block_cache``.
    ``iter_time`` has one entry per step -- a Heun step's covers both evaluations -- with one device synchronisation per step.
    Guidance: ``extra_args["guidance"]`` (the dict of ``_guidance_options``) replaces the step launch of a guided evaluation by dk_guided_cfg_step
    (two small launches for the per-image moments, then the step) for "rescale" and "apg", and under an interval runs the evaluations outside it
    on the prompt rows alone: where the guidedness changes, ``_set_rows`` re-prepares the engine, the first-block cache (if on) is reset and that
    evaluation computes whatever the policy says, and the update is dk_lms_cfg_step with cfg_on = 0 on the first n_img token rows.  APG's momentum
    buffer is allocated here and never initialised: the first guided evaluation of a stretch does not read it.  What ran goes to
    ``model.guidance_record``.
    Skip-layer guidance: ``extra_args["skip_layer_guidance"]`` ({"scale", "layers", "interval"}, ``_skip_layer_options``) gives the evaluations of
    ``sampler.slg_rows`` a third row group, forked inside the engine, and dk_slg_cfg_step as their update; ``_set_rows`` re-prepares the engine where the
    window begins and ends, and the engine's skip layers are off again when the loop returns or raises.  What ran goes to ``model.skip_layer_record``.
    Stochastic samplers: a plan with noise terms (``step_plan("euler_a" | "sde", ...)``) needs ``extra_args["noise_seeds"]``, one integer in [0, 2^64)
    per image; its rows end in dk_noisy_cfg_step, which draws the noise in the launch."""
    plan = list(plan)
    guide = None if extra_args is None else extra_args.get("guidance")
    slg = None if extra_args is None else extra_args.get("skip_layer_guidance")
    seeds = None if extra_args is None else extra_args.get("noise_seeds")
    grows = guidance_rows(plan, None if guide is None else guide["interval"])
    lp = _loop_setup(model, x, sigmas, extra_args, guided=grows[0].guided if grows else True)
    if guide is not None and not lp.cfg_on:
        raise ValueError("extra_args['guidance'] needs classifier-free guidance (cfg_weight > 0)")
    if slg is not None and not lp.cfg_on:
        raise ValueError("extra_args['skip_layer_guidance'] needs classifier-free guidance (cfg_weight > 0)")
    pag = None if extra_args is None else extra_args.get("perturbed_attention_guidance")
    if pag is not None and slg is not None:
        raise ValueError("extra_args holds both 'skip_layer_guidance' and 'perturbed_attention_guidance': the engine forks one row group")
    if pag is not None and not lp.cfg_on:
        raise ValueError("extra_args['perturbed_attention_guidance'] needs classifier-free guidance (cfg_weight > 0)")
    if (slg is not None or pag is not None) and lp.policy is not None:
        raise ValueError(("skip-layer" if slg is not None else "perturbed-attention") +
                         " guidance cannot run together with block_cache: there is no cache policy for a forked row group yet")
    if lp.policy is not None and not all(r.ends_step for r in plan):
        raise ValueError(_HEUN_BLOCK_CACHE)
    if any(not 0 <= r.index < len(lp.sigmas) - 1 for r in plan):
        raise ValueError("the plan evaluates the model outside the schedule (or at its last entry): build it with sampler.step_plan on these sigmas")
    if lp.forked is None:
        try:
            return _step_loop(model, lp, plan, grows, guide, noise_seeds=seeds)
        finally:
            if lp.control is not None:  # (the main engine's taps are off again when the loop returns or raises)
                lp.mm.set_control_taps(None)
    window = lp.forked["interval"]  # (None, perturbed-attention guidance only: every guided row)
    srows = [bool(g.guided) for g in grows] if window is None else slg_rows(plan, grows, *window)
    try:
        return _step_loop(model, lp, plan, grows, guide, srows=srows, noise_seeds=seeds)
    finally:
        lp.set_fork(False)


_FLOWEDIT_REFUSED = {
    "mask": "mask_path (inpainting)", "block_cache": "block_cache", "guidance": "a guidance mode other than 'cfg' or guidance_interval",
    "skip_layer_guidance": "skip-layer guidance", "perturbed_attention_guidance": "perturbed-attention guidance", "controlnet": "a ControlNet",
    "ip_adapter": "an IP-Adapter", "reference": "a reference image", "condition": "channel-concatenated conditioning (condition=)"}


def _flowedit_refusal(what: str) -> str:
    return f"an edit (edit_source_text) cannot run together with {what}: the edit loop has its own step launch and its own batch rows"


def sample_flowedit(model: CFGDenoiser, x_src: Tensor, sigmas, n_max: int, n_min: int = 0, n_avg: int = 1, extra_args=None):
    """The edit phase of FlowEdit (Kulikov et al. 2024, "Inversion-Free Text-Based Editing Using Pre-Trained Flow Models"; no reference counterpart;
    the statement is ``sampler.flowedit_reference``).  ``x_src``: f32 [n_img, h, w, C], the encoded source images after ``process_in``; ``sigmas``:
    the whole schedule, of which the steps T - n_max .. T - n_min - 1 run here (the first T - n_max run nothing at all).
    ``extra_args``: ``conditioning`` / ``pooled_conditioning`` laid out per image for 2 n_img images, the source rows first -- [src | tar] x n_img
    each, and with ``cfg_weight`` > 0 (the TARGET's CFG weight) [src+ | tar+ | src- | tar-]; ``edit_source_cfg``: the source's CFG weight (default:
    the target's); ``edit_guidance_rows``: one distilled-guidance value per batch row (FLUX.1-dev), or None; ``noise_seeds``: one integer in [0, 2^64)
    per image.  Every model evaluation runs the source and the target of one draw as batch rows of one ``forward_tokens`` and is followed by one
    launch of dk_flowedit_step, which updates Z, draws the next noise in registers (Philox stream 1) and writes the next inputs; the prime launch
    in front forms the first ones.  One device synchronisation per outer step.
    Returns (Z, Zt, iter_time).  n_min == 0: Z is the result (the last launch forms its inputs at sigma 0, where Zt is Z but for the rounding of
    x_src + (Z - x_src)).  Otherwise Zt is the state at sigmas[T - n_min] that the ordinary loop
    (``sample_euler`` / ``sample_steps`` on sigmas[T - n_min:], the target rows alone) takes to sigma 0.  ``model.flowedit_record`` says what ran."""
    from . import ops
    from .sampler import flowedit_plan
    extra_args = {} if extra_args is None else dict(extra_args)
    for key, what in _FLOWEDIT_REFUSED.items():
        if extra_args.get(key) is not None:
            raise ValueError(_flowedit_refusal(what))
    w_src = extra_args.pop("edit_source_cfg", None)
    grows = extra_args.pop("edit_guidance_rows", None)
    seeds = extra_args.pop("noise_seeds", None)
    plan = flowedit_plan(sigmas, n_max, n_min, n_avg)
    pipe = model.model
    x_src = x_src.to(pipe.device, torch.float32).contiguous()
    n_img = x_src.shape[0]
    if seeds is None or len(seeds) != n_img:
        raise ValueError(f"sample_flowedit: extra_args['noise_seeds'] must hold one seed per image ({n_img})")
    cfg_on = float(extra_args.get("cfg_weight", 7.5)) > 0
    if not cfg_on and not pipe._IS_FLUX:
        raise ValueError("an edit on the SD3 family needs classifier-free guidance on both sides (cfg_weight > 0 and edit_source_cfg > 0)")
    lp = _loop_setup(model, torch.cat([x_src, x_src], 0), sigmas, extra_args)  # (2 n_img images: the source rows and the target rows)
    mm, pcfg = lp.mm, pipe.mmdit_config
    w_tar = lp.cfg_weight
    w_src = w_tar if w_src is None else float(w_src)
    try:
        if grows is not None:  # (the table again, with a guidance value per batch row)
            mm.cache_modulation_params(lp.pooled, lp.timesteps, guidance_rows=grows)
        z, zt = x_src.clone(), torch.empty_like(x_src)
        sd = ops.seed_tensor(seeds, x_src.device)
        tok, out = lp.tok, lp.out
        iter_time, t0, evals = [], None, 0
        for r in plan:
            t0 = time.perf_counter() if t0 is None else t0
            if not r.prime:
                mm.forward_tokens(tok, None, r.index, tokens_out=out)
                evals += 1
            ops.flowedit_step(z, x_src, None if r.prime else out, tok, zt, n_img, cfg_on, pcfg.patch_size, int(pcfg.patchify_via_reshape), c=r.c,
                              sigma_in=r.sigma_in, seeds=sd, draw=r.draw, w_src=w_src, w_tar=w_tar, prime=r.prime)
            if r.ends_step:
                torch.cuda.synchronize(pipe.device)
                iter_time.append(round(time.perf_counter() - t0, 3))
                t0 = None
    finally:
        if grows is not None:  # (the engine outlives the call: the scalar again)
            mm.clear_guidance_rows()
    model.flowedit_record = {"n_max": int(n_max), "n_min": int(n_min), "n_avg": int(n_avg), "model_evals": evals, "draws": len(plan),
                             "rows": int(tok.shape[0]), "source_cfg": w_src if cfg_on else None, "target_cfg": w_tar if cfg_on else None,
                             "guidance_rows": None if grows is None else [float(g) for g in grows]}
    model.clear_cache()
    return z, zt, iter_time
