"""Shape/dtype presets for the denoising hot path.

Mirrors the fields of the reference's ``MMDiTConfig`` / ``VAEDecoderConfig``
(reference: python/src/diffusionkit/mlx/config.py:19-71, 74-111, 126-132) that the
hot path reads.  Fields the reference declares but never reads
(``upcast_*_blocks``, ``low_memory_mode``) are dropped.  ``guidance_embed`` is the reference's field
(config.py:71,109): its FLUX_DEV preset sets it, but model_io.py:109,756 selects FLUX_SCHNELL for the
FLUX.1-dev checkpoint (quirk Q7) and the one call site (mmdit.py:219-220) cannot run; MODEL_CONFIG keeps that
default, and ``FLUX_DEV`` below enables the published FLUX.1-dev conditioning for callers who pass it.
``weight_dtype`` has no reference counterpart: "fp8_e4m3" runs the block Linears on the fp8 MFMA
(BASELINE.json configs[3]).
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from enum import Enum
from typing import Optional, Tuple


class PositionalEncoding(Enum):
    LearnedInputEmbedding = 1
    PreSDPARope = 2


@dataclass(frozen=True)
class MMDiTConfig:
    num_heads: int = 24
    depth_multimodal: int = 24
    depth_unified: int = 0
    parallel_mlp_for_unified_blocks: bool = True
    mlp_ratio: int = 4
    vae_latent_dim: int = 16
    layer_norm_eps: float = 1e-6
    pos_embed_type: PositionalEncoding = PositionalEncoding.LearnedInputEmbedding
    rope_axes_dim: Optional[Tuple[int, ...]] = None
    rope_theta: int = 10000
    use_qk_norm: bool = False
    hidden_size_override: Optional[int] = None
    max_latent_resolution: int = 192
    patch_size: int = 2
    patchify_via_reshape: bool = False
    pooled_text_embed_dim: int = 2048
    token_level_text_embed_dim: int = 4096
    frequency_embed_dim: int = 256
    max_period: int = 10000
    # dtype the timestep embedding is evaluated in (reference config.dtype, quirk Q2)
    dtype: str = "bfloat16"
    guidance_embed: bool = False
    # storage / MFMA dtype of the transformer blocks' Linear weights: "bfloat16", or "fp8_e4m3" (per-output-channel scales,
    # MX-fp8 activations quantised on the fly; FLUX geometry only: head_dim 128, text length a multiple of 128 -- any image token count)
    weight_dtype: str = "bfloat16"
    # fp8 precision policy (only read with weight_dtype = "fp8_e4m3"): the Linears of the first n double-stream blocks stay bf16 --
    # an error made in the first blocks travels through all the others (measured dB per block: DESIGN.md section 4)
    fp8_bf16_double_blocks: int = 0
    # element type of the MMDiT's weights, activations and token / text / pooled I/O: "bfloat16", or "float16" -- the reference's dtype for
    # Stable Diffusion 3 (config.py:77-79); SD3-family geometry only (validate_activation_dtype)
    activation_dtype: str = "bfloat16"
    # channel-concatenated conditioning (FLUX.1 Fill: 320, Canny / Depth: 64; 0: none): x_embedder.proj.weight has patch_dim + condition_features
    # columns, and a condition token row of that width rides into every model evaluation (MMDiTEngine.cache_condition); FLUX family only
    condition_features: int = 0
    # MMDiT-X (Stable Diffusion 3.5 medium; no reference counterpart): the first n double blocks carry a second self-attention over the image
    # tokens alone (x_block.attn2), fed by a second modulation of the block's LayerNorm and gated by a ninth adaLN row; SD3 family only
    # (validate_dual_attention)
    dual_attention_blocks: int = 0
    # SD3 ControlNet (the layout of diffusers' SD3ControlNetModel; no reference counterpart): this configuration is the ControlNet, not a model --
    # ``depth_multimodal`` joint blocks with their own embedders, a second patch embedder for the control image (pos_embed_input) and one
    # Linear(h, h) per block (controlnet_blocks), no final layer; SD3 family only (validate_control_net)
    control_net: bool = False
    # FLUX ControlNet (the layout of diffusers' FluxControlNetModel; no reference counterpart): this configuration is the ControlNet --
    # ``depth_multimodal`` double and ``depth_unified`` single blocks with their own embedders, a second patch embedder for the control image
    # (controlnet_x_embedder), one Linear(h, h) per double block (controlnet_blocks) and per single block (controlnet_single_blocks), no final
    # layer; FLUX family only (validate_control_net_flux).  ``control_net`` stays the SD3 family's field
    control_net_flux: bool = False

    @property
    def hidden_size(self) -> int:
        return self.hidden_size_override or (64 * self.depth_multimodal)

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_heads

    @property
    def patch_dim(self) -> int:
        return self.patch_size ** 2 * self.vae_latent_dim

    @property
    def is_flux(self) -> bool:
        return self.depth_unified > 0

    def param_count(self) -> int:
        """Approximate parameter count (linear weights only): 12 h^2 per stream / single block (+ 4 h^2 for the second attention of a
        dual block) plus the adaLN Linears."""
        h = self.hidden_size
        per_stream = (4 + 2 * self.mlp_ratio) * h * h
        n = (2 * self.depth_multimodal + self.depth_unified) * per_stream
        n += self.dual_attention_blocks * 4 * h * h
        n += self.num_modulation_rows() * h * h
        n += (self.token_level_text_embed_dim + self.pooled_text_embed_dim + self.frequency_embed_dim + 2 * h) * h
        return n

    def num_modulation_rows(self) -> int:
        """Number of hidden-size rows of adaLN output per (timestep, batch row).

        double block: 6 (image; 9 for a dual-attention block) + 6 (text); the last SD3 block's text stream has 2
        (reference mmdit.py:64-65,424-427); single block: 3; final layer: 2.
        """
        n = 0
        for i in range(self.depth_multimodal):
            skip_txt = (i == self.depth_multimodal - 1) and self.depth_unified < 1
            n += (9 if i < self.dual_attention_blocks else 6) + (2 if skip_txt else 6)
        n += 3 * self.depth_unified
        n += 0 if self.control_net or self.control_net_flux else 2  # (a ControlNet has no final layer)
        return n


# reference config.py:78-80 (fp16 there; bf16 here by default, float16_config(SD3_2b) runs it in the reference's dtype)
SD3_2b = MMDiTConfig(depth_multimodal=24, num_heads=24, dtype="float16")

# reference config.py:74-76
SD3_8b = MMDiTConfig(depth_multimodal=38, num_heads=38, use_qk_norm=True)

# Stable Diffusion 3.5 medium (no reference counterpart; published model definition: MMDiT-X, depth 24, 384^2 position table, QK-RMSNorm, the
# first 13 joint blocks with a second, image-only attention)
SD3_5_MEDIUM = MMDiTConfig(depth_multimodal=24, num_heads=24, use_qk_norm=True, max_latent_resolution=384, dual_attention_blocks=13)


def validate_dual_attention(cfg: MMDiTConfig) -> None:
    """0 <= dual_attention_blocks <= depth_multimodal, and above 0 only on the SD3 family with bf16 / fp16 Linears: depth_unified == 0, no
    fp8 weights (the rule dk_mmdit_set_dual_attention enforces)."""
    n = cfg.dual_attention_blocks
    if not (0 <= n <= cfg.depth_multimodal):
        raise ValueError(f"dual_attention_blocks = {n}: must lie in [0, depth_multimodal = {cfg.depth_multimodal}]")
    if n > 0 and (cfg.depth_unified != 0 or cfg.weight_dtype == "fp8_e4m3"):
        raise ValueError("dual_attention_blocks needs the SD3 family (MMDiT-X): depth_unified == 0 and no fp8 Linears")


# The InstantX SD3-medium ControlNets (Canny / Pose / Tile; diffusers' SD3ControlNetModel): six joint blocks of SD3-medium's width.  The width is
# the MODEL's (24 * 64), not 64 * depth
SD3_CONTROLNET_6 = replace(SD3_2b, depth_multimodal=6, hidden_size_override=SD3_2b.hidden_size, control_net=True)


def validate_control_net(cfg: MMDiTConfig) -> None:
    """``control_net`` needs SD3 geometry: the learned positional table, depth_unified == 0, no fp8 Linears, no dual attention blocks, no
    condition width (the rule dk_mmdit_set_control_net enforces)."""
    if not cfg.control_net:
        return
    if (cfg.pos_embed_type != PositionalEncoding.LearnedInputEmbedding or cfg.depth_unified != 0 or cfg.weight_dtype == "fp8_e4m3"
            or cfg.dual_attention_blocks != 0 or cfg.condition_features != 0):
        raise ValueError("control_net needs the SD3 family: the learned positional table, depth_unified == 0, no fp8 Linears, no dual attention "
                         "blocks and no condition width")


# reference config.py:82-95
FLUX_SCHNELL = MMDiTConfig(
    num_heads=24,
    depth_multimodal=19,
    depth_unified=38,
    parallel_mlp_for_unified_blocks=True,
    hidden_size_override=3072,
    patchify_via_reshape=True,
    pos_embed_type=PositionalEncoding.PreSDPARope,
    rope_axes_dim=(16, 56, 56),
    pooled_text_embed_dim=768,
    use_qk_norm=True,
    dtype="bfloat16",
)


# reference config.py:97-111 (declared there, never selected: quirk Q7)
FLUX_DEV = replace(FLUX_SCHNELL, guidance_embed=True)

# FLUX.1 Fill / Canny / Depth (no reference counterpart): FLUX.1-dev by keys and widths but for img_in, [3072, 64 + 320] / [3072, 64 + 64] -- the
# condition latent's 64 patch features (Fill: + the 8 x 8-unshuffled mask's 256) concatenated to the latent's on the feature axis
FLUX_FILL_DEV = replace(FLUX_DEV, condition_features=320)
FLUX_CONTROL_DEV = replace(FLUX_DEV, condition_features=64)


def validate_control_net_flux(cfg: MMDiTConfig) -> None:
    """``control_net_flux`` needs FLUX geometry: RoPE and no learned positional table, at least one double block, bfloat16 activations, no fp8
    Linears, no dual attention blocks, no condition width, and not ``control_net`` (the SD3 form) at the same time -- the rule
    dk_mmdit_set_flux_control_net enforces."""
    if not cfg.control_net_flux:
        return
    if cfg.control_net:
        raise ValueError("control_net_flux and control_net cannot both be set: control_net is the SD3 family's ControlNet")
    if (cfg.pos_embed_type != PositionalEncoding.PreSDPARope or cfg.depth_multimodal < 1 or cfg.depth_unified < 0
            or cfg.weight_dtype == "fp8_e4m3" or cfg.activation_dtype != "bfloat16" or cfg.dual_attention_blocks != 0 or cfg.condition_features != 0):
        raise ValueError("control_net_flux needs the FLUX family: RoPE without a learned positional table, at least one double block, bfloat16 "
                         "activations, no fp8 Linears, no dual attention blocks and no condition width")


def flux_controlnet_config(n_double: int, n_single: int, base: Optional[MMDiTConfig] = None) -> MMDiTConfig:
    """The FLUX ControlNet with ``n_double`` double and ``n_single`` single blocks for a model like ``base`` (default FLUX_DEV): the model's
    width, heads, RoPE axes and embedders (the guidance embedding of a guidance-distilled model included), its own depths.  FLUX ControlNets have
    no canonical depth: the caller names it."""
    base = FLUX_DEV if base is None else base
    if n_double < 1 or n_single < 0:
        raise ValueError(f"a FLUX ControlNet has n_double >= 1 and n_single >= 0 blocks, got ({n_double}, {n_single})")
    out = replace(base, depth_multimodal=n_double, depth_unified=n_single, hidden_size_override=base.hidden_size, control_net_flux=True,
                  condition_features=0, weight_dtype="bfloat16", fp8_bf16_double_blocks=0)
    validate_control_net_flux(out)
    return out


@dataclass(frozen=True)
class IPAdapterConfig:
    """FLUX IP-Adapter (XLabs-AI flux-ip-adapter as diffusers runs it; no reference counterpart): a pipeline-level setting, not part of the model's
    configuration -- the engine learns ``ip_adapter_tokens`` and ``ip_adapter_dim`` through dk_mmdit_set_ip_adapter.  The projection model maps one
    image embedding [embed_dim] to ``ip_adapter_tokens`` tokens of ``ip_adapter_dim`` features (Linear, reshape, LayerNorm); every double block of
    the model owns a to_k_ip / to_v_ip Linear(ip_adapter_dim -> hidden_size)."""
    ip_adapter_tokens: int = 4
    ip_adapter_dim: int = 4096
    embed_dim: int = 768  # CLIP ViT-L/14 image_embeds
    norm_eps: float = 1e-5


FLUX_IP_ADAPTER = IPAdapterConfig()


def validate_ip_adapter(cfg: MMDiTConfig, ip: IPAdapterConfig) -> None:
    """The rule dk_mmdit_set_ip_adapter enforces, in the host's words: the FLUX family with bf16 Linears and activations, head_dim 128, QK-norm, no
    condition width, not a ControlNet; 1 .. 16 tokens of a width that is a multiple of 64."""
    if cfg.pos_embed_type != PositionalEncoding.PreSDPARope or cfg.depth_multimodal < 1:
        raise ValueError("an IP-Adapter needs the FLUX family: RoPE without a learned positional table and at least one double block "
                         "(SD3 and SD3.5 IP-Adapters are not built)")
    if cfg.weight_dtype == "fp8_e4m3":
        raise ValueError("an IP-Adapter cannot be combined with fp8 Linears: the fp8 LayerNorm kernels take no tap")
    if cfg.activation_dtype != "bfloat16" or cfg.head_dim != 128 or not cfg.use_qk_norm:
        raise ValueError("an IP-Adapter needs bfloat16 activations, head_dim 128 and QK-norm weights")
    if cfg.condition_features != 0 or cfg.control_net or cfg.control_net_flux or cfg.dual_attention_blocks != 0:
        raise ValueError("an IP-Adapter cannot be combined with a condition width, a ControlNet configuration or dual attention blocks")
    if not 1 <= ip.ip_adapter_tokens <= 16:
        raise ValueError(f"ip_adapter_tokens = {ip.ip_adapter_tokens}: must lie in [1, 16] (InstantX's 128-token adapters are not built)")
    if ip.ip_adapter_dim <= 0 or ip.ip_adapter_dim % 64 != 0 or ip.embed_dim <= 0:
        raise ValueError(f"ip_adapter_dim = {ip.ip_adapter_dim}: must be a positive multiple of 64, with a positive embed_dim")


def tiny_ip_adapter(tokens: int = 4, dim: int = 256, embed_dim: int = 64) -> IPAdapterConfig:
    """IP-Adapter small enough for the CPU oracle beside a ``tiny_flux`` model (whose hidden size its K / V Linears take from the model)."""
    return IPAdapterConfig(ip_adapter_tokens=tokens, ip_adapter_dim=dim, embed_dim=embed_dim)


def validate_condition_features(cfg: MMDiTConfig) -> None:
    """0, or a positive multiple of 64 on a configuration without the learned positional table and with bf16 activations (the rule
    dk_mmdit_set_condition_width enforces)."""
    n = cfg.condition_features
    if n == 0:
        return
    if n < 0 or n % 64 != 0:
        raise ValueError(f"condition_features = {n}: must be 0 or a positive multiple of 64")
    if cfg.pos_embed_type == PositionalEncoding.LearnedInputEmbedding or cfg.activation_dtype != "bfloat16":
        raise ValueError("condition_features needs the FLUX family: no learned positional table (the x_embedder launch's residual operand carries "
                         "the condition's share) and bfloat16 activations")


# fp8 precision policy of the FLUX family, measured at full depth on MI355X (scripts/fp8_policy_gpu.py, profiles/r05_fp8_policy_gpu.log:
# Euler direction of teacher-forced steps 1 / 2 / 49 / 50 against the fp32 oracle): every double-stream block kept in bf16 buys ~0.27 dB and
# costs ~0.36 ms per step; 12 of the 19 put every step at >= 35 dB (35.1 - 36.4 dB, 46.3 ms per step against 41.8 all-fp8 / 61.6 bf16)
FLUX_FP8_QUALITY_BLOCKS = 12


def fp8_config(cfg: MMDiTConfig, policy: str = "quality") -> MMDiTConfig:
    """``cfg`` on the fp8 path (BASELINE.json configs[3]).  policy "quality" (default): the first FLUX_FP8_QUALITY_BLOCKS double-stream blocks keep
    bf16 Linears (>= 35 dB per step, SURVEY.md section 8c iii); "speed": every block Linear in fp8 (31.6 - 32.5 dB per step)."""
    if policy not in ("quality", "speed"):
        raise ValueError(f"unknown fp8 policy {policy!r} (quality | speed)")
    # (reject here what dk_mmdit_create would only reject later -- the fp8 kernels are FLUX geometry: head_dim 128, width a multiple of 256)
    if cfg.head_dim != 128 or cfg.hidden_size % 256 != 0:
        raise ValueError(f"fp8_config: the fp8 path needs head_dim 128 and hidden_size % 256 == 0 (got {cfg.head_dim}, {cfg.hidden_size}); "
                         "at run time the text length must be a multiple of 128, the image size is free")
    n = min(FLUX_FP8_QUALITY_BLOCKS, cfg.depth_multimodal) if policy == "quality" else 0
    out = replace(cfg, weight_dtype="fp8_e4m3", fp8_bf16_double_blocks=n)
    validate_fp8_policy(out)
    return out


def validate_activation_dtype(cfg: MMDiTConfig) -> None:
    """``activation_dtype`` is "bfloat16" or "float16"; float16 is the SD3 family's: head_dim == 64, depth_unified == 0 and no fp8 Linears
    (the rule dk_mmdit_set_activation_dtype enforces -- the D = 128 attention kernels, the single-stream blocks' fused launches and the fp8 path
    are bf16 only)."""
    if cfg.activation_dtype not in ("bfloat16", "float16"):
        raise ValueError(f"unknown activation_dtype {cfg.activation_dtype!r} (bfloat16 | float16)")
    if cfg.activation_dtype == "bfloat16":
        return
    if cfg.head_dim != 64 or cfg.depth_unified != 0:
        raise ValueError(f"activation_dtype float16 needs SD3-family geometry: head_dim == 64 and depth_unified == 0 "
                         f"(got head_dim {cfg.head_dim}, depth_unified {cfg.depth_unified})")
    if cfg.weight_dtype == "fp8_e4m3":
        raise ValueError("activation_dtype float16 cannot be combined with weight_dtype fp8_e4m3 (the fp8 path's activations are bf16 / MX-fp8)")


def float16_config(cfg: MMDiTConfig) -> MMDiTConfig:
    """``cfg`` with float16 weights and activations (the reference's dtype for SD3); raises ValueError for any other family."""
    out = replace(cfg, activation_dtype="float16")
    validate_activation_dtype(out)
    return out


def validate_fp8_policy(cfg: MMDiTConfig) -> None:
    """0 <= fp8_bf16_double_blocks <= depth_multimodal (the C engine and weights.pack_mmdit clamp independently: a value outside the range
    would only surface as a missing-tensor error)."""
    n = cfg.fp8_bf16_double_blocks
    if not (0 <= n <= cfg.depth_multimodal):
        raise ValueError(f"fp8_bf16_double_blocks = {n}: must lie in [0, depth_multimodal = {cfg.depth_multimodal}]")


def tiny_flux(depth_multimodal: int = 2, depth_unified: int = 2, heads: int = 2,
              head_dim: int = 128, text_dim: int = 256, pooled: int = 64, condition_features: int = 0) -> MMDiTConfig:
    """FLUX-shaped config small enough for the CPU oracle (head_dim stays 128 so the
    RoPE axes (16,56,56) and the D=128 attention kernel are the production ones)."""
    return replace(
        FLUX_SCHNELL,
        num_heads=heads,
        depth_multimodal=depth_multimodal,
        depth_unified=depth_unified,
        hidden_size_override=heads * head_dim,
        token_level_text_embed_dim=text_dim,
        pooled_text_embed_dim=pooled,
        condition_features=condition_features,
    )


def tiny_flux_controlnet(n_double: int = 2, n_single: int = 2, heads: int = 2, head_dim: int = 128, text_dim: int = 256, pooled: int = 64,
                         guidance_embed: bool = False) -> MMDiTConfig:
    """FLUX-ControlNet-shaped config for a ``tiny_flux`` model of the same ``heads`` and ``head_dim`` (the widths must agree: the taps are added
    to its stream); ``n_single`` may be 0."""
    base = replace(tiny_flux(1, 1, heads, head_dim, text_dim, pooled), guidance_embed=guidance_embed)
    return flux_controlnet_config(n_double, n_single, base)


def tiny_sd3(depth: int = 2, heads: int = 4, text_dim: int = 256, pooled: int = 64,
             max_res: int = 24) -> MMDiTConfig:
    """SD3-shaped config (head_dim 64, learned pos-emb, conv patchify)."""
    return replace(
        SD3_2b,
        num_heads=heads,
        depth_multimodal=depth,
        hidden_size_override=heads * 64,
        token_level_text_embed_dim=text_dim,
        pooled_text_embed_dim=pooled,
        max_latent_resolution=max_res,
    )


def tiny_sd3_controlnet(depth: int = 2, heads: int = 4, text_dim: int = 256, pooled: int = 64, max_res: int = 24) -> MMDiTConfig:
    """SD3-ControlNet-shaped config for a ``tiny_sd3`` model of the same ``heads`` (the widths must agree: the taps are added to its stream)."""
    return replace(tiny_sd3(depth, heads, text_dim, pooled, max_res), control_net=True)


def tiny_sd35m(depth: int = 3, heads: int = 4, dual: int = 2, text_dim: int = 256, pooled: int = 64, max_res: int = 24) -> MMDiTConfig:
    """SD3.5-medium-shaped config (MMDiT-X: head_dim 64, QK-RMSNorm, learned pos-emb, the first ``dual`` blocks with the second attention; the
    defaults put a plain block and the text-skipping last block behind the dual ones)."""
    return replace(
        SD3_5_MEDIUM,
        num_heads=heads,
        depth_multimodal=depth,
        dual_attention_blocks=dual,
        hidden_size_override=heads * 64,
        token_level_text_embed_dim=text_dim,
        pooled_text_embed_dim=pooled,
        max_latent_resolution=max_res,
    )


@dataclass(frozen=True)
class VAEDecoderConfig:
    """reference config.py:126-132"""
    in_channels: int = 16
    out_channels: int = 3
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 3
    resnet_groups: int = 32
    group_norm_eps: float = 1e-5  # MLX nn.GroupNorm default (vae.py:34,72,78,381)
    # element type of the weights, the activations and the raw output: "bfloat16", or "float16" -- the reference's decoder dtype for Stable
    # Diffusion 3 (mlx/__init__.py:108-113,483-484); see float16_vae_config
    dtype: str = "bfloat16"


@dataclass(frozen=True)
class VAEEncoderConfig:
    """reference config.py:135-140 (the image -> latent half used by img2img, vae.py:404-467)"""
    in_channels: int = 3
    out_channels: int = 32  # mean | logvar of the 16 latent channels
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    resnet_groups: int = 32
    group_norm_eps: float = 1e-5
    # element type of the weights, the activations and the 16-bit moments: "bfloat16" or "float16".  The reference keeps its encoder in fp32
    # (load_vae_encoder(float16=False), mlx/__init__.py:116): float16 is the closer of the two 16-bit forms, not the reference's dtype
    dtype: str = "bfloat16"


VAE_DTYPES = ("bfloat16", "float16")


def validate_vae_dtype(dtype: str) -> str:
    """``dtype`` of a VAE half: "bfloat16" or "float16"; anything else raises ValueError."""
    if dtype not in VAE_DTYPES:
        raise ValueError(f"unknown VAE dtype {dtype!r} (bfloat16 | float16)")
    return dtype


def float16_vae_config(cfg, dtype: str = "float16"):
    """``cfg`` (VAEDecoderConfig or VAEEncoderConfig) with float16 weights and activations -- or, with ``dtype``, in that element type;
    unknown values raise ValueError.  Any channel plan: the VAE's fp16 kernels have no geometry rule."""
    if not isinstance(cfg, (VAEDecoderConfig, VAEEncoderConfig)):
        raise ValueError(f"float16_vae_config takes a VAEDecoderConfig or VAEEncoderConfig, got {type(cfg).__name__}")
    return replace(cfg, dtype=validate_vae_dtype(dtype))


def tiny_vae_encoder() -> VAEEncoderConfig:
    return VAEEncoderConfig(block_out_channels=(64, 64, 128, 128), layers_per_block=1)


def tiny_vae() -> VAEDecoderConfig:
    return VAEDecoderConfig(block_out_channels=(64, 64, 128, 128), layers_per_block=1)


# reference mlx/__init__.py:37-53
MMDIT_CKPT = {
    "argmaxinc/mlx-stable-diffusion-3-medium": "argmaxinc/mlx-stable-diffusion-3-medium",
    "argmaxinc/mlx-stable-diffusion-3.5-large": "argmaxinc/mlx-stable-diffusion-3.5-large",
    "argmaxinc/mlx-stable-diffusion-3.5-large-4bit-quantized": "argmaxinc/mlx-stable-diffusion-3.5-large-4bit-quantized",
    "argmaxinc/mlx-FLUX.1-schnell": "argmaxinc/mlx-FLUX.1-schnell",
    "argmaxinc/mlx-FLUX.1-schnell-4bit-quantized": "argmaxinc/mlx-FLUX.1-schnell-4bit-quantized",
    "argmaxinc/mlx-FLUX.1-dev": "argmaxinc/mlx-FLUX.1-dev",
    "stabilityai/stable-diffusion-3.5-medium": "stabilityai/stable-diffusion-3.5-medium",  # (no reference counterpart: local checkpoints only)
}

T5_MAX_LENGTH = {
    "argmaxinc/mlx-stable-diffusion-3-medium": 512,
    "argmaxinc/mlx-stable-diffusion-3.5-large": 512,
    "argmaxinc/mlx-stable-diffusion-3.5-large-4bit-quantized": 512,
    "argmaxinc/mlx-FLUX.1-schnell": 256,
    "argmaxinc/mlx-FLUX.1-schnell-4bit-quantized": 256,
    "argmaxinc/mlx-FLUX.1-dev": 512,
    "stabilityai/stable-diffusion-3.5-medium": 512,
}

# reference model_io.py:104-111 (_CONFIG): which MMDiT preset a model_version selects
MODEL_CONFIG = {
    "argmaxinc/mlx-stable-diffusion-3-medium": SD3_2b,
    "argmaxinc/mlx-FLUX.1-schnell": FLUX_SCHNELL,
    "argmaxinc/mlx-FLUX.1-schnell-4bit-quantized": FLUX_SCHNELL,
    "argmaxinc/mlx-FLUX.1-dev": FLUX_SCHNELL,  # quirk Q7: dev runs without guidance embedding
    "argmaxinc/mlx-stable-diffusion-3.5-large": SD3_8b,
    "argmaxinc/mlx-stable-diffusion-3.5-large-4bit-quantized": SD3_8b,
    "stabilityai/stable-diffusion-3.5-medium": SD3_5_MEDIUM,
}

# Skip-layer guidance: the sampling recipe published with a model version (Stability's sd3_infer.py and diffusers' StableDiffusion3Pipeline run
# SD3.5-medium with it): the double blocks the third evaluation skips, the scale of its term and the (start, stop) fractions of the schedule.
# Every other SD3 version must name its layers (pipeline ``skip_layers=``).  Arithmetic only: no SD3.5-medium checkpoint has been run here.
SKIP_LAYER_GUIDANCE = {
    "stabilityai/stable-diffusion-3.5-medium": {"layers": (7, 8, 9), "scale": 2.5, "interval": (0.01, 0.2)},
}
