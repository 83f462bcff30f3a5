"""``python -m diffusionkit_amd.cli``: the reference's ``diffusionkit-cli`` in front of this build's
pipelines.  Flags, defaults, the per-model height / width / shift tables, the FLUX "no CFG" rule, the benchmark-mode
warm-up and the error behaviour follow python/src/diffusionkit/mlx/scripts/generate_images.py:15-187.

There is no hub access on an MI355X box, so checkpoints are named explicitly: ``--fp8 quality|speed`` selects the fp8 path (config.fp8_config)
of the FLUX versions; ``--local-ckpt`` is the MMDiT
``.safetensors`` (as in the reference) and ``--ckpt KEY=PATH`` adds the other parts (``vae_decoder``, ``vae_encoder``, ``clip_l``,
``clip_g``, ``t5``, ``t5_tokenizer``; ``tokenizer_l`` / ``tokenizer_g`` take ``vocab.json,merges.txt``).  Parts that are not named
run on seeded synthetic weights / synthetic conditioning and the log line says so -- useful for timing, not for pictures.
"""
from __future__ import annotations

import argparse
import logging
from typing import Dict, Optional, Sequence

logger = logging.getLogger("diffusionkit_amd.cli")

# generate_images.py:15-38
HEIGHT = {
    "argmaxinc/mlx-stable-diffusion-3-medium": 512,
    "argmaxinc/mlx-stable-diffusion-3.5-large": 1024,
    "argmaxinc/mlx-stable-diffusion-3.5-large-4bit-quantized": 1024,
    "argmaxinc/mlx-FLUX.1-schnell": 512,
    "argmaxinc/mlx-FLUX.1-schnell-4bit-quantized": 512,
    "argmaxinc/mlx-FLUX.1-dev": 512,
    "stabilityai/stable-diffusion-3.5-medium": 1024,  # (no reference counterpart; runs from --local-ckpt)
}
WIDTH = dict(HEIGHT)
SHIFT = {k: (1.0 if "FLUX" in k else 3.0) for k in HEIGHT}


def build_parser(model_versions: Sequence[str]) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="diffusionkit-amd-cli",
                                description="Generate images from a text (and an optional image) prompt on MI355X")
    p.add_argument("--prompt", required=True, help="Text prompt")
    p.add_argument("--image-path", type=str, default=None, help="Path to the image prompt")
    p.add_argument("--model-version", choices=tuple(model_versions), default="argmaxinc/mlx-FLUX.1-schnell",
                   help="Diffusion model version, e.g. FLUX-1.schnell, stable-diffusion-3-medium")
    p.add_argument("--steps", type=int, default=50, help="Number of diffusion steps.")
    p.add_argument("--cfg", type=float, default=5.0, help="Classifier-free guidance weight")
    p.add_argument("--negative_prompt", default="", help="Negative text prompt")
    p.add_argument("--preload-models", action="store_true", help="Accepted for compatibility: models are always resident in HBM.")
    p.add_argument("--output-path", "-o", default="out.png", help="Path to save the output image.")
    p.add_argument("--seed", type=int, help="Seed for the random number generator.")
    p.add_argument("--verbose", "-v", action="store_true", help="Print detailed information.")
    p.add_argument("--shift", type=float, help="Shift for diffusion sampling")
    p.add_argument("--t5", action="store_true", help="Engages T5 for stronger text embeddings.")
    p.add_argument("--height", type=int, help="Height of the output image")
    p.add_argument("--width", type=int, help="Width of the output image")
    p.add_argument("--no-low-memory-mode", action="store_false", dest="low_memory_mode",
                   help="Accepted for compatibility: nothing is offloaded with 288 GB of HBM.")
    p.add_argument("--benchmark-mode", action="store_true", help="Warm the kernels up with a one-step run first.")
    p.add_argument("--denoise", type=float, default=0.0,
                   help="Denoising factor when an input image is provided. (between 0.0 and 1.0)")
    p.add_argument("--mask-path", type=str, default=None,
                   help="Inpainting mask for --image-path (first channel; 255 = repaint, 0 = keep; resized to the image with NEAREST).")
    p.add_argument("--no-composite", action="store_true",
                   help="With --mask-path: do not paste the kept pixels of the input image back over the decoded image.")
    p.add_argument("--reference-image-path", type=str, default=None,
                   help="Reference-image conditioning in FLUX.1 Kontext's token layout (FLUX versions only): the image is VAE-encoded and its "
                        "tokens ride behind the image tokens at RoPE index 1. Sides must be multiples of 16 pixels; it is not resized. "
                        "Verified as arithmetic only: no Kontext checkpoint has been run here.")
    p.add_argument("--condition", choices=("fill", "control"), default=None,
                   help="Channel-concatenated conditioning (FLUX versions only): 'fill' is FLUX.1 Fill's layout (the masked image's latent and the "
                        "mask ride into every model evaluation; needs --condition-image-path and --condition-mask-path), 'control' FLUX.1 Canny / "
                        "Depth's (a prepared control image; --condition-image-path). The checkpoint's img_in must be 384 / 128 columns wide. "
                        "Verified as arithmetic only: no such checkpoint has been run here.")
    p.add_argument("--condition-image-path", type=str, default=None,
                   help="With --condition: the image to fill in, or the prepared control image (edges, depth). Its sides must equal "
                        "--height / --width; it is not resized.")
    p.add_argument("--condition-mask-path", type=str, default=None,
                   help="With --condition fill: the mask (first channel; 255 = repaint, 0 = keep, values between are passed on as they are). "
                        "Same size as the image; not resized.")
    p.add_argument("--block-cache", type=float, default=None, metavar="THRESHOLD",
                   help="First-block cache: skip the blocks behind block 0 in steps where block 0's effect moved by less than THRESHOLD "
                        "(a float >= 0, relative to the last computed step). Published implementations use about 0.1 for FLUX; no value "
                        "has been validated here on a real checkpoint.")
    p.add_argument("--sampler", choices=("euler", "heun", "ab2", "euler_a", "sde"), default=None,
                   help="Integrator of the step loop. euler (default): first order, one model evaluation per step. heun: second order, two "
                        "evaluations per step but the last (not together with --block-cache). ab2: second order, one evaluation per step. "
                        "The orders are checked on an analytic problem, not on a trained checkpoint. euler_a: ancestral Euler for rectified flows "
                        "(k-diffusion's sample_euler_ancestral_RF), first order, re-noises a share --sampler-eta of every step. sde: diffusers' "
                        "stochastic_sampling, which re-draws all of the noise every step; offered as the published definition and nothing more. Both "
                        "draw their noise on the GPU from the image's seed; neither has been run on a trained checkpoint here.")
    p.add_argument("--sampler-eta", type=float, default=None, metavar="ETA",
                   help="With --sampler euler_a: the share of each step that is re-noised, in [0, 1] (default 1; 0 is euler).")
    p.add_argument("--guidance", choices=("cfg", "rescale", "apg"), default=None,
                   help="How the prompt and the negative prediction are combined (models with --cfg > 0 only). cfg (default): neg + w (pos - neg). "
                        "rescale: the same, scaled towards the prompt prediction's standard deviation (--guidance-rescale). apg: adaptive "
                        "projected guidance (--apg-eta, --apg-norm-threshold, --apg-momentum). Verified as arithmetic only: no setting has "
                        "been validated on a trained checkpoint here.")
    p.add_argument("--guidance-rescale", type=float, default=None, metavar="PHI", help="rescale: blend factor in [0, 1] (default 0.7).")
    p.add_argument("--apg-eta", type=float, default=None, metavar="ETA", help="apg: weight of the component parallel to the prediction (default 0).")
    p.add_argument("--apg-norm-threshold", type=float, default=None, metavar="R",
                   help="apg: clip the norm of the guidance direction to R per image (default 0 = off).")
    p.add_argument("--apg-momentum", type=float, default=None, metavar="BETA",
                   help="apg: momentum of the guidance direction over the guided evaluations (default 0; the paper uses -0.5).")
    p.add_argument("--guidance-interval", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="Guide only the model evaluations whose sigma lies in [LO, HI]; the others run on the prompt alone, at half the batch.")
    p.add_argument("--slg-scale", type=float, nargs="?", const=True, default=None, metavar="SCALE",
                   help="Skip-layer guidance (SD3 versions with --cfg > 0): add SCALE times (prompt prediction - prediction with layers skipped) in "
                        "the steps of --slg-interval. Without a value: the scale published with the model version (2.5 for Stable Diffusion 3.5 "
                        "medium). Not together with --block-cache. Verified as arithmetic only: no SD3.5-medium checkpoint has been run here.")
    p.add_argument("--skip-layers", type=int, nargs="+", default=None, metavar="BLOCK",
                   help="With --slg-scale: the double blocks the third evaluation skips (default: the model version's published ones, 7 8 9 for "
                        "Stable Diffusion 3.5 medium; other versions must name them).")
    p.add_argument("--slg-interval", type=float, nargs=2, default=None, metavar=("START", "STOP"),
                   help="With --slg-scale: step i of n takes the term iff n START < i < n STOP (default: the model version's published 0.01 0.2, "
                        "else 0 1).")
    p.add_argument("--pag-scale", type=float, default=None, metavar="S",
                   help="Perturbed-attention guidance (SD3 versions with --cfg > 0): add S times (prompt prediction - prediction with the attention "
                        "of --pag-layers perturbed: image queries see the text and themselves only). Needs --pag-layers. Not together with "
                        "--slg-scale or --block-cache. Verified as arithmetic only: no checkpoint has been run here.")
    p.add_argument("--pag-layers", type=int, nargs="+", default=None, metavar="BLOCK", help="With --pag-scale: the double blocks whose attention is perturbed.")
    p.add_argument("--pag-interval", type=float, nargs=2, default=None, metavar=("START", "STOP"),
                   help="With --pag-scale: step i of n takes the term iff n START < i < n STOP (default: every guided step).")
    p.add_argument("--controlnet", type=str, default=None, metavar="PATH",
                   help="An SD3 ControlNet in the layout of diffusers' SD3ControlNetModel (the InstantX SD3-medium Canny / Pose / Tile files; SD3 "
                        "versions, not Stable Diffusion 3.5 medium) or, with a FLUX version and --controlnet-blocks, a FLUX ControlNet in the layout "
                        "of diffusers' FluxControlNetModel: a .safetensors file. Needs --controlnet-image-path. Not together with "
                        "--block-cache, --slg-scale, --pag-scale or --fp8. Verified as arithmetic only: the key table has not been run against a real file.")
    p.add_argument("--controlnet-blocks", type=int, nargs=2, default=None, metavar=("N_DOUBLE", "N_SINGLE"),
                   help="With --controlnet and a FLUX model version: the ControlNet is a FLUX one in the layout of diffusers' FluxControlNetModel with this "
                        "many double and single blocks (FLUX ControlNets have no canonical depth; e.g. 5 10). Not together with --fp8, --block-cache, "
                        "--reference-image-path or --condition. Union-mode and XLabs files are refused. Verified as arithmetic only: the key table "
                        "has not been run against a real file.")
    p.add_argument("--controlnet-image-path", type=str, default=None, metavar="IMG",
                   help="With --controlnet: the prepared control image (edges, pose, ...). Its sides must equal --height / --width: it is not resized.")
    p.add_argument("--controlnet-scale", type=float, default=None, metavar="S", help="With --controlnet: the scale of the ControlNet's residuals (default 1.0).")
    p.add_argument("--controlnet-interval", type=float, nargs=2, default=None, metavar=("START", "STOP"),
                   help="With --controlnet: step i of n is controlled iff i / n >= START and (i + 1) / n <= STOP (default: every step).")
    p.add_argument("--edit-source-prompt", type=str, default=None, metavar="TEXT",
                   help="FlowEdit (Kulikov et al. 2024): edit --image-path with the plain checkpoint. TEXT describes the image as it is, --prompt what "
                        "it should become. The defaults of the flags below are the paper's settings as recalled and have not been verified. Not "
                        "together with --denoise, --mask-path, --block-cache, guidance modes, --slg-scale, --pag-scale, --controlnet, --ip-adapter, "
                        "--reference-image-path or --condition. Verified as arithmetic only: no trained checkpoint has been run here.")
    p.add_argument("--edit-steps", type=int, nargs=2, default=None, metavar=("N_MAX", "N_MIN"),
                   help="With --edit-source-prompt: the edit covers the steps T - N_MAX .. T - N_MIN - 1 of the --steps = T schedule; the last N_MIN steps "
                        "are ordinary sampling with the target prompt (0 <= N_MIN < N_MAX <= T; default: 33/50 of T for SD3, 24/28 for FLUX, and 0).")
    p.add_argument("--edit-n-avg", type=int, default=None, metavar="N", help="With --edit-source-prompt: noise draws averaged per step (default 1).")
    p.add_argument("--edit-source-cfg", type=float, default=None, metavar="W",
                   help="With --edit-source-prompt: the source side's CFG weight (SD3 versions; --cfg is the target's; default 3.5) or distilled-guidance "
                        "value (FLUX.1-dev; default 1.5). Refused for FLUX.1-schnell, which has no guidance embedding.")
    p.add_argument("--local-ckpt", default=None, type=str, help="Path to the local mmdit checkpoint.")
    p.add_argument("--ckpt", action="append", default=[], metavar="KEY=PATH",
                   help="Further local checkpoint parts (vae_decoder, vae_encoder, clip_l, clip_g, t5, t5_tokenizer, "
                        "tokenizer_l=vocab.json,merges.txt, tokenizer_g=...). Repeatable.")
    p.add_argument("--ip-adapter", type=str, default=None, metavar="PATH",
                   help="A FLUX IP-Adapter in XLabs-AI's layout (flux-ip-adapter: 4 tokens from a CLIP ViT-L/14 image embedding, decoupled attention "
                        "in the double blocks): a .safetensors file; FLUX versions only. Needs --ip-adapter-embeds. Not together with --fp8, "
                        "--controlnet, --block-cache, --reference-image-path or --condition (the CLI runs FLUX without CFG). The vision tower is not part of this "
                        "build. Verified as arithmetic only: the key table has not been run against a real file.")
    p.add_argument("--ip-adapter-embeds", type=str, default=None, metavar="FILE.npy",
                   help="With --ip-adapter: the prepared CLIP image embedding(s) of the image prompt, a .npy array [768] or [1, 768].")
    p.add_argument("--ip-adapter-scale", type=float, default=None, metavar="S", help="With --ip-adapter: the scale of the adapter's output (default 1.0).")
    p.add_argument("--fp8", choices=("quality", "speed"), default=None,
                   help="Run the transformer blocks on the fp8 MFMA path (FLUX versions only). quality: the first double-stream "
                        "blocks keep bf16 Linears; speed: every block Linear in fp8.")
    p.add_argument("--activation-dtype", choices=("bfloat16", "float16"), default="bfloat16",
                   help="Element type of the MMDiT's weights and activations. float16 is the reference's dtype for Stable Diffusion 3 "
                        "(SD3 versions only); the text encoders stay bfloat16, the VAE has --vae-dtype.")
    p.add_argument("--vae-dtype", choices=("bfloat16", "float16"), default=None,
                   help="Element type of the VAE decoder and (img2img) encoder; default bfloat16. float16 is the reference's decoder dtype "
                        "for Stable Diffusion 3 (not for FLUX); accepted for every model version.")
    p.add_argument("--device", default=None, help="HIP device, e.g. cuda:0 (default: the current device)")
    return p


def checkpoint_dict(local_ckpt: Optional[str], parts: Sequence[str]) -> Optional[Dict[str, object]]:
    """--local-ckpt / --ckpt KEY=PATH -> the ``local_ckpt`` dict DiffusionPipeline takes."""
    out: Dict[str, object] = {}
    if local_ckpt:
        out["mmdit"] = local_ckpt
    for kv in parts:
        if "=" not in kv:
            raise ValueError(f"--ckpt expects KEY=PATH, got {kv!r}")
        k, v = kv.split("=", 1)
        out[k] = tuple(v.split(",")) if k.startswith("tokenizer_") else v
    return out or None


def resolve(args) -> dict:
    """The argument post-processing of generate_images.py:114-150, as data (so that it can be tested without a GPU)."""
    cfg = args.cfg
    if "FLUX" in args.model_version and cfg > 0.0:
        logger.warning(f"Disabling CFG for {args.model_version} model.")
        cfg = 0.0
    if args.denoise < 0.0 or args.denoise > 1.0:
        raise ValueError("Denoising factor must be between 0.0 and 1.0")
    height = args.height or HEIGHT[args.model_version]
    width = args.width or WIDTH[args.model_version]
    assert height % 16 == 0, f"Height must be divisible by 16 ({height}/16={height/16})"
    assert width % 16 == 0, f"Width must be divisible by 16 ({width}/16={width/16})"
    r = {"cfg": cfg, "shift": args.shift or SHIFT[args.model_version], "height": height, "width": width,
         "flux": "FLUX" in args.model_version, "low_memory_mode": args.low_memory_mode and not args.benchmark_mode}
    if getattr(args, "fp8", None):
        # (config.fp8_config raises a ValueError for the SD3 geometries: head_dim 64)
        from .config import MODEL_CONFIG, fp8_config
        r["mmdit_config"] = fp8_config(MODEL_CONFIG[args.model_version], args.fp8)
    if getattr(args, "activation_dtype", "bfloat16") != "bfloat16":
        # (config.float16_config raises a ValueError for the FLUX geometries and together with --fp8)
        from .config import MODEL_CONFIG, float16_config
        float16_config(r.get("mmdit_config", MODEL_CONFIG[args.model_version]))
        r["activation_dtype"] = args.activation_dtype
    if getattr(args, "vae_dtype", None) is not None:  # (a key only when the flag is given)
        from .config import validate_vae_dtype
        r["vae_dtype"] = validate_vae_dtype(args.vae_dtype)
    if getattr(args, "mask_path", None) is not None:  # (keys only when the flags are given)
        if args.image_path is None:
            raise ValueError("--mask-path needs --image-path")
        r["mask_path"] = args.mask_path
    if getattr(args, "no_composite", False):
        r["composite"] = False
    if getattr(args, "reference_image_path", None) is not None:  # (a key only when the flag is given)
        if "FLUX" not in args.model_version:
            raise ValueError(f"--reference-image-path needs a FLUX model version (RoPE positions tell the reference from the image), not {args.model_version}")
        r["reference_image_path"] = args.reference_image_path
    kind = getattr(args, "condition", None)
    cond_image, cond_mask = getattr(args, "condition_image_path", None), getattr(args, "condition_mask_path", None)
    if kind is not None or cond_image is not None or cond_mask is not None:  # (keys only when the flags are given)
        from .pipeline import check_condition_args
        check_condition_args(kind, cond_image, cond_mask, r.get("reference_image_path"), "FLUX" in args.model_version)
        r["condition"] = kind
        r["condition_image_path"] = cond_image
        if cond_mask is not None:
            r["condition_mask_path"] = cond_mask
    if getattr(args, "block_cache", None) is not None:  # (a key only when the flag is given)
        if not args.block_cache >= 0.0:
            raise ValueError("Block cache threshold must be a float >= 0")
        r["block_cache"] = args.block_cache
    if getattr(args, "sampler", None) is not None:  # (a key only when the flag is given)
        if args.sampler == "heun" and "block_cache" in r:
            raise ValueError("--sampler heun cannot run together with --block-cache (two model evaluations per step have no cache policy yet); "
                             "use --sampler ab2")
        r["sampler"] = args.sampler
    if getattr(args, "sampler_eta", None) is not None:  # (a key only when the flag is given)
        if r.get("sampler") != "euler_a":
            raise ValueError("--sampler-eta belongs to --sampler euler_a")
        if not 0.0 <= args.sampler_eta <= 1.0:
            raise ValueError("--sampler-eta must lie in [0, 1]")
        r["sampler_eta"] = args.sampler_eta
    for flag, key in GUIDANCE_FLAGS.items():  # (keys only when the flags are given)
        v = getattr(args, flag, None)
        if v is not None:
            if cfg <= 0.0:
                raise ValueError(f"--{flag.replace('_', '-')} needs classifier-free guidance (--cfg > 0), which {args.model_version} runs without")
            r[key] = tuple(v) if flag == "guidance_interval" else v
    if "guidance_rescale" in r and not 0.0 <= r["guidance_rescale"] <= 1.0:
        raise ValueError("--guidance-rescale must lie in [0, 1]")
    if "guidance_interval" in r and not r["guidance_interval"][0] <= r["guidance_interval"][1]:
        raise ValueError("--guidance-interval expects LO <= HI")
    scale, layers, window = (getattr(args, k, None) for k in ("slg_scale", "skip_layers", "slg_interval"))
    if scale is not None or layers is not None or window is not None:  # (keys only when the flags are given)
        from .config import MODEL_CONFIG
        from .pipeline import _skip_layer_options
        opts = _skip_layer_options(scale, layers, window, args.model_version, r.get("mmdit_config", MODEL_CONFIG[args.model_version]),
                                   "FLUX" in args.model_version, cfg, r.get("block_cache"))
        r.update(skip_layer_guidance=opts["scale"], skip_layers=opts["layers"], skip_layer_interval=opts["interval"])
    pag = tuple(getattr(args, k, None) for k in ("pag_scale", "pag_layers", "pag_interval"))
    if any(v is not None for v in pag):  # (keys only when the flags are given)
        from .config import MODEL_CONFIG
        from .pipeline import _perturbed_attention_options
        mcfg = r.get("mmdit_config", MODEL_CONFIG[args.model_version])
        opts = _perturbed_attention_options(*pag, mcfg, "FLUX" in args.model_version, cfg, r.get("block_cache"), r.get("reference_image_path"),
                                            r.get("condition"), r.get("skip_layer_guidance"))
        r.update(pag_scale=opts["scale"], pag_layers=opts["layers"], pag_interval=opts["interval"])
    cn = {k: getattr(args, k, None) for k in ("controlnet", "controlnet_image_path", "controlnet_scale", "controlnet_interval", "controlnet_blocks")}
    if any(v is not None for v in cn.values()):  # (keys only when the flags are given)
        from .config import MODEL_CONFIG
        mcfg = r.get("mmdit_config", MODEL_CONFIG[args.model_version])
        if cn["controlnet"] is None:
            raise ValueError("--controlnet-image-path / --controlnet-scale / --controlnet-interval / --controlnet-blocks need --controlnet")
        if cn["controlnet_image_path"] is None:
            raise ValueError("--controlnet needs --controlnet-image-path: the ControlNet was trained to see a control image")
        blocks = getattr(args, "controlnet_blocks", None)
        if "FLUX" in args.model_version:
            if blocks is None:
                raise ValueError(f"--controlnet without --controlnet-blocks needs an SD3 model version (diffusers' SD3ControlNetModel), not "
                                 f"{args.model_version}: a FLUX ControlNet (diffusers' FluxControlNetModel) names its depths, --controlnet-blocks N_DOUBLE N_SINGLE")
            from dataclasses import replace
            from .config import flux_controlnet_config
            for key, flag in (("reference_image_path", "--reference-image-path"), ("condition", "--condition")):
                if r.get(key) is not None:
                    raise ValueError(f"--controlnet cannot run together with {flag}")
            r["controlnet_config"] = flux_controlnet_config(int(blocks[0]), int(blocks[1]), replace(mcfg, weight_dtype="bfloat16", fp8_bf16_double_blocks=0))
        elif blocks is not None:
            raise ValueError(f"--controlnet-blocks is the FLUX family's (diffusers' FluxControlNetModel), not {args.model_version}'s: an SD3 ControlNet's "
                             "depth is its preset's")
        if mcfg.dual_attention_blocks > 0:
            raise ValueError(f"--controlnet cannot run with {args.model_version}: its dual attention blocks have no tap form")
        if getattr(args, "fp8", None):
            raise ValueError("--controlnet cannot run together with --fp8")
        for key, flag in (("block_cache", "--block-cache"), ("skip_layer_guidance", "--slg-scale"), ("pag_scale", "--pag-scale")):
            if r.get(key) is not None:
                raise ValueError(f"--controlnet cannot run together with {flag}")
        if cn["controlnet_interval"] is not None and not cn["controlnet_interval"][0] <= cn["controlnet_interval"][1]:
            raise ValueError("--controlnet-interval expects START <= STOP")
        r["controlnet_ckpt"] = cn["controlnet"]
        r["controlnet_image_path"] = cn["controlnet_image_path"]
        if cn["controlnet_scale"] is not None:
            r["controlnet_scale"] = cn["controlnet_scale"]
        if cn["controlnet_interval"] is not None:
            r["controlnet_interval"] = tuple(cn["controlnet_interval"])
    ipa = {k: getattr(args, k, None) for k in ("ip_adapter", "ip_adapter_embeds", "ip_adapter_scale")}
    if any(v is not None for v in ipa.values()):
        if ipa["ip_adapter"] is None:
            raise ValueError("--ip-adapter-embeds / --ip-adapter-scale need --ip-adapter")
        if ipa["ip_adapter_embeds"] is None:
            raise ValueError("--ip-adapter needs --ip-adapter-embeds: the prepared image embedding of the image prompt (the vision tower is not built)")
        if "FLUX" not in args.model_version:
            raise ValueError(f"--ip-adapter needs a FLUX model version, not {args.model_version}: SD3 and SD3.5 IP-Adapters are not built")
        if getattr(args, "fp8", None):
            raise ValueError("--ip-adapter cannot run together with --fp8")
        for key, flag in (("controlnet_ckpt", "--controlnet"), ("block_cache", "--block-cache"), ("reference_image_path", "--reference-image-path"),
                          ("condition", "--condition")):
            if r.get(key) is not None:
                raise ValueError(f"--ip-adapter cannot run together with {flag}")
        r["ip_adapter_ckpt"] = ipa["ip_adapter"]
        r["ip_adapter_image_embeds"] = ipa["ip_adapter_embeds"]
        if ipa["ip_adapter_scale"] is not None:
            r["ip_adapter_scale"] = ipa["ip_adapter_scale"]
    ed = {k: getattr(args, k, None) for k in ("edit_source_prompt", "edit_steps", "edit_n_avg", "edit_source_cfg")}
    if any(v is not None for v in ed.values()):  # (keys only when the flags are given)
        if ed["edit_source_prompt"] is None:
            raise ValueError("--edit-steps / --edit-n-avg / --edit-source-cfg need --edit-source-prompt")
        if args.image_path is None:
            raise ValueError("--edit-source-prompt needs --image-path: the image to edit")
        if args.denoise != 0.0:  # (the flag's default: not given)
            raise ValueError("--edit-source-prompt cannot run together with --denoise: --edit-steps says which part of the schedule the edit covers")
        for key, flag in (("mask_path", "--mask-path"), ("block_cache", "--block-cache"), ("guidance", "--guidance"),
                          ("guidance_interval", "--guidance-interval"), ("skip_layer_guidance", "--slg-scale"), ("pag_scale", "--pag-scale"),
                          ("controlnet_ckpt", "--controlnet"), ("ip_adapter_ckpt", "--ip-adapter"), ("reference_image_path", "--reference-image-path"),
                          ("condition", "--condition")):
            if r.get(key) is not None and not (key == "guidance" and r[key] == "cfg"):
                raise ValueError(f"--edit-source-prompt cannot run together with {flag}")
        if ed["edit_steps"] is not None:
            from .sampler import check_flowedit
            r["edit_steps"] = check_flowedit(args.steps, ed["edit_steps"][0], ed["edit_steps"][1], 1)[:2]
        if ed["edit_n_avg"] is not None:
            if ed["edit_n_avg"] < 1:
                raise ValueError("--edit-n-avg must be at least 1")
            r["edit_n_avg"] = ed["edit_n_avg"]
        if ed["edit_source_cfg"] is not None:
            from .config import MODEL_CONFIG
            if "FLUX" in args.model_version and not r.get("mmdit_config", MODEL_CONFIG[args.model_version]).guidance_embed:
                raise ValueError(f"--edit-source-cfg is the source's distilled-guidance value on FLUX: {args.model_version} has no guidance embedding")
            r["edit_source_cfg"] = ed["edit_source_cfg"]
        r["edit_source_text"] = ed["edit_source_prompt"]
    return r


EDIT_KEYS = ("edit_source_text", "edit_steps", "edit_n_avg", "edit_source_cfg")  # the same, FlowEdit
SKIP_LAYER_KEYS = ("skip_layer_guidance", "skip_layers", "skip_layer_interval")  # keywords of generate_image that ``resolve`` sets together
PAG_KEYS = ("pag_scale", "pag_layers", "pag_interval")  # the same, perturbed-attention guidance
CONTROLNET_KEYS = ("controlnet_image_path", "controlnet_scale", "controlnet_interval")  # the same, SD3 ControlNet (the constructor takes controlnet_ckpt)
IP_ADAPTER_KEYS = ("ip_adapter_image_embeds", "ip_adapter_scale")  # the same, FLUX IP-Adapter (the constructor takes ip_adapter_ckpt)
# argparse destination -> keyword of generate_image
GUIDANCE_FLAGS = {"guidance": "guidance", "guidance_rescale": "guidance_rescale", "apg_eta": "apg_eta", "apg_norm_threshold": "apg_norm_threshold",
                  "apg_momentum": "apg_momentum", "guidance_interval": "guidance_interval"}


def main(argv: Optional[Sequence[str]] = None, pipeline_overrides: Optional[dict] = None):
    """Returns (PIL.Image, log) after saving the image.  ``pipeline_overrides`` are extra keyword arguments for the pipeline
    constructor (tests pass tiny configs through it)."""
    from .config import MMDIT_CKPT
    args = build_parser(tuple(MMDIT_CKPT.keys())).parse_args(argv)
    logging.basicConfig(level=logging.INFO if args.verbose else logging.WARNING)
    r = resolve(args)
    from .pipeline import DiffusionPipeline, FluxPipeline
    pipeline_class = FluxPipeline if r["flux"] else DiffusionPipeline
    extra = dict(pipeline_overrides or {})
    if args.fp8:  # (a config of the caller's is put on the fp8 path like the model version's own)
        from .config import fp8_config
        extra["mmdit_config"] = fp8_config(extra["mmdit_config"], args.fp8) if extra.get("mmdit_config") is not None else r["mmdit_config"]
    if "activation_dtype" in r:
        extra["activation_dtype"] = r["activation_dtype"]
    if "vae_dtype" in r:
        extra["vae_dtype"] = r["vae_dtype"]
    if "condition" in r:
        extra["condition"] = r["condition"]
    if "controlnet_ckpt" in r:
        extra["controlnet_ckpt"] = r["controlnet_ckpt"]
    if "controlnet_config" in r:
        extra["controlnet_config"] = r["controlnet_config"]
    if "ip_adapter_ckpt" in r:
        extra["ip_adapter_ckpt"] = r["ip_adapter_ckpt"]
    cond_kw = {key: r[key] for key in ("condition_image_path", "condition_mask_path", *CONTROLNET_KEYS, *IP_ADAPTER_KEYS) if key in r}
    if "ip_adapter_image_embeds" in cond_kw:  # (the file is read here: generate_image takes arrays)
        import numpy as np
        cond_kw["ip_adapter_image_embeds"] = np.load(cond_kw["ip_adapter_image_embeds"], allow_pickle=False)
    sd = pipeline_class(w16=True, shift=r["shift"], use_t5=args.t5, model_version=args.model_version,
                        low_memory_mode=r["low_memory_mode"], a16=True, local_ckpt=checkpoint_dict(args.local_ckpt, args.ckpt),
                        device=args.device, **extra)
    logger.info(f"Output image resolution will be {r['height']}x{r['width']}")
    latent_size = (r["height"] // 8, r["width"] // 8)
    if args.benchmark_mode:
        logger.info("Running in benchmark mode. Warming up the models. (generated latents will be discarded)")
        sd.generate_image(args.prompt, cfg_weight=r["cfg"], num_steps=1, seed=args.seed, negative_text=args.negative_prompt,
                          latent_size=latent_size, verbose=False, **cond_kw)
        logger.info("Benchmark mode: Warming up the models done.")
    image, log = sd.generate_image(args.prompt, cfg_weight=r["cfg"], num_steps=args.steps, seed=args.seed,
                                   negative_text=args.negative_prompt, latent_size=latent_size, image_path=args.image_path,
                                   denoise=1.0 if "edit_source_text" in r else args.denoise, verbose=args.verbose, mask_path=r.get("mask_path"),
                                   composite=r.get("composite", True), block_cache=r.get("block_cache"), sampler=r.get("sampler"),
                                   **{key: r[key] for key in (*GUIDANCE_FLAGS.values(), "reference_image_path", *SKIP_LAYER_KEYS, *PAG_KEYS, "sampler_eta", *EDIT_KEYS)
                                      if key in r},
                                   **cond_kw)
    if log["text_encoding"].get("synthetic"):
        logger.warning("no text-encoder checkpoints were named (--ckpt clip_l=... t5=...): the conditioning is synthetic")
    image.save(args.output_path)
    logger.info(f"Saved the image to {args.output_path}")
    return image, log


if __name__ == "__main__":
    main()
