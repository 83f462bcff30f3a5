"""Host-side mirrors of the reference's model objects, backed by libdk_hip.so.

``MMDiTEngine`` mirrors ``MMDiT`` (python/src/diffusionkit/mlx/mmdit.py:22-266:
``cache_modulation_params`` / ``__call__``), ``VAEDecoderEngine`` mirrors ``VAEDecoder``
(python/src/diffusionkit/mlx/vae.py:336-401).  PyTorch is used for device memory and
streams only; every FLOP runs in the HIP library.  There is no fallback path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import _lib
from .config import MMDiTConfig, PositionalEncoding, VAEDecoderConfig

Tensor = torch.Tensor
_EMBED_DTYPE = {"bfloat16": 0, "float16": 1, "float32": 2}
_ACT_DTYPE = {"bfloat16": (0, torch.bfloat16), "float16": (1, torch.float16)}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _require_cuda(t: Tensor, name: str, dtype=None):
    if not t.is_cuda:
        raise _lib.DkHipError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise _lib.DkHipError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.DkHipError(f"{name} must be contiguous")


class MMDiTEngine:
    """Drop-in for the reference ``MMDiT`` module on the hot path."""

    def __init__(self, config: MMDiTConfig, packed_weights: Dict[str, Tensor], ip_adapter=None):
        """``ip_adapter``: a ``config.IPAdapterConfig`` when ``packed_weights`` also holds ``weights.pack_ip_adapter``'s tensors (FLUX family)."""
        self.lib = _lib.load()
        self.config = config
        dev0 = next(iter(packed_weights.values())).device
        if dev0.type == "cuda":
            _lib.ensure_attention_workspace(dev0)  # (the key-split workgroups of the D = 128 attention kernel)
        c = _lib.dk_mmdit_config()
        c.num_heads, c.depth_multimodal, c.depth_unified = config.num_heads, config.depth_multimodal, config.depth_unified
        c.hidden_size, c.mlp_ratio = config.hidden_size, config.mlp_ratio
        c.vae_latent_dim, c.patch_size = config.vae_latent_dim, config.patch_size
        c.patchify_via_reshape = int(config.patchify_via_reshape)
        c.use_qk_norm = int(config.use_qk_norm)
        c.use_rope = int(config.pos_embed_type == PositionalEncoding.PreSDPARope)
        axes = list(config.rope_axes_dim or ())
        for i, a in enumerate(axes):
            c.rope_axes_dim[i] = a
        c.n_rope_axes, c.rope_theta = len(axes), config.rope_theta
        c.use_pos_embed = int(config.pos_embed_type == PositionalEncoding.LearnedInputEmbedding)
        c.max_latent_resolution = config.max_latent_resolution
        c.pooled_text_embed_dim = config.pooled_text_embed_dim
        c.token_level_text_embed_dim = config.token_level_text_embed_dim
        c.frequency_embed_dim, c.max_period = config.frequency_embed_dim, config.max_period
        c.embed_dtype = _EMBED_DTYPE[config.dtype]
        c.layer_norm_eps = config.layer_norm_eps
        c.guidance_embed = int(config.guidance_embed)
        if config.weight_dtype not in ("bfloat16", "fp8_e4m3"):
            raise _lib.DkHipError(f"unknown weight_dtype {config.weight_dtype!r} (bfloat16 | fp8_e4m3)")
        c.fp8_linears = int(config.weight_dtype == "fp8_e4m3")
        if c.fp8_linears:
            from .config import validate_fp8_policy
            validate_fp8_policy(config)
        c.fp8_bf16_double_blocks = int(config.fp8_bf16_double_blocks) if c.fp8_linears else 0
        h = C.c_void_p()
        _lib.check(self.lib.dk_mmdit_create(C.byref(c), C.byref(h)), "dk_mmdit_create")
        self._h = h
        from .config import validate_activation_dtype
        try:
            validate_activation_dtype(config)
        except ValueError as e:
            raise _lib.DkHipError(str(e)) from None
        # element type of the weights and of tokens / text / pooled at this boundary (set before the first bind; 0 is the engine's default)
        code, self.dtype = _ACT_DTYPE[config.activation_dtype]
        _lib.check(self.lib.dk_mmdit_set_activation_dtype(self._h, code), "dk_mmdit_set_activation_dtype")
        # channel-concatenated conditioning: x_embedder's weight is read as [h, patch_dim + condition_features]; dk_mmdit_bind sees a bare
        # pointer, so the column count is checked here, before anything is bound (a narrower weight would be read out of bounds)
        from .config import validate_condition_features
        try:
            validate_condition_features(config)
        except ValueError as e:
            raise _lib.DkHipError(str(e)) from None
        self.condition_features = int(config.condition_features)
        xw = packed_weights.get("x_embedder.proj.weight")
        if xw is not None and (xw.dim() != 2 or xw.shape[1] != config.patch_dim + self.condition_features):
            raise _lib.DkHipError(f"x_embedder.proj.weight is {tuple(xw.shape)}: the configuration (patch_dim {config.patch_dim}, condition_features "
                                  f"{self.condition_features}) needs {config.patch_dim + self.condition_features} columns")
        if self.condition_features:
            _lib.check(self.lib.dk_mmdit_set_condition_width(self._h, self.condition_features), "dk_mmdit_set_condition_width")
        self._cond_cached = False
        # MMDiT-X dual-attention blocks: the 9-row image modules and the attn2 weights of the first n blocks (before anything is bound)
        from .config import validate_dual_attention
        try:
            validate_dual_attention(config)
        except ValueError as e:
            raise _lib.DkHipError(str(e)) from None
        if config.dual_attention_blocks:
            _lib.check(self.lib.dk_mmdit_set_dual_attention(self._h, int(config.dual_attention_blocks)), "dk_mmdit_set_dual_attention")
        # SD3 ControlNet: this engine is the ControlNet (no final layer, a second patch embedder, one tap Linear per block); set before the first bind
        from .config import validate_control_net
        try:
            validate_control_net(config)
        except ValueError as e:
            raise _lib.DkHipError(str(e)) from None
        self.control_net = bool(config.control_net)
        if self.control_net:
            _lib.check(self.lib.dk_mmdit_set_control_net(self._h, 1), "dk_mmdit_set_control_net")
            for name, cols in [("pos_embed_input.proj.weight", config.patch_dim)] + [(f"controlnet_blocks.{i}.weight", config.hidden_size)
                                                                                      for i in range(config.depth_multimodal)]:
                t = packed_weights.get(name)  # (dk_mmdit_bind sees bare pointers: the shapes are checked here)
                if t is None or tuple(t.shape) != (config.hidden_size, cols):
                    raise _lib.DkHipError(f"{name}: a control-net engine needs a [{config.hidden_size}, {cols}] tensor, got "
                                          f"{None if t is None else tuple(t.shape)}")
        # FLUX ControlNet: the same on FLUX geometry, with tap Linears behind the double and behind the single blocks
        from .config import validate_control_net_flux
        try:
            validate_control_net_flux(config)
        except ValueError as e:
            raise _lib.DkHipError(str(e)) from None
        self.control_net_flux = bool(config.control_net_flux)
        if self.control_net_flux:
            _lib.check(self.lib.dk_mmdit_set_flux_control_net(self._h, 1), "dk_mmdit_set_flux_control_net")
            names = ([("controlnet_x_embedder.proj.weight", config.patch_dim)]
                     + [(f"controlnet_blocks.{i}.weight", config.hidden_size) for i in range(config.depth_multimodal)]
                     + [(f"controlnet_single_blocks.{i}.weight", config.hidden_size) for i in range(config.depth_unified)])
            for name, cols in names:
                t = packed_weights.get(name)  # (dk_mmdit_bind sees bare pointers: the shapes are checked here)
                if t is None or tuple(t.shape) != (config.hidden_size, cols):
                    raise _lib.DkHipError(f"{name}: a FLUX control-net engine needs a [{config.hidden_size}, {cols}] tensor, got "
                                          f"{None if t is None else tuple(t.shape)}")
            self.control_net = True  # (what cache_control_image / control_forward ask)
        self._ctrl_cached = False
        # FLUX IP-Adapter: token count and width before the weights resolve; the stacked K / V matrix is read through bare pointers, so its layout
        # is checked here
        self.ip_adapter = ip_adapter
        self.ip_scale = 0.0
        self._ip_cached = False
        if ip_adapter is not None:
            from .config import validate_ip_adapter
            try:
                validate_ip_adapter(config, ip_adapter)
            except ValueError as e:
                raise _lib.DkHipError(str(e)) from None
            nd, hh, cc = config.depth_multimodal, config.hidden_size, ip_adapter.ip_adapter_dim
            kvw, kvb = packed_weights.get("ip_adapter.kv.weight"), packed_weights.get("ip_adapter.kv.bias")
            if kvw is None or kvb is None or tuple(kvw.shape) != (nd * 2 * hh, cc) or tuple(kvb.shape) != (nd * 2 * hh,) or not kvw.is_contiguous():
                raise _lib.DkHipError(f"ip_adapter.kv.weight / .bias: an engine with an IP-Adapter needs the stacked [{nd * 2 * hh}, {cc}] matrix and "
                                      f"its [{nd * 2 * hh}] bias (weights.pack_ip_adapter)")
            _lib.check(self.lib.dk_mmdit_set_ip_adapter(self._h, int(ip_adapter.ip_adapter_tokens), int(cc)), "dk_mmdit_set_ip_adapter")
        # ``set_control_taps`` / ``set_flux_control_taps``: (taps tensor, scale), kept alive while the engine reads it; None: off
        self.control_taps = None
        self.weights = packed_weights  # keep the device tensors alive
        for name, t in packed_weights.items():
            want = torch.uint8 if name.endswith(".weight_fp8") else torch.float32 if name.endswith(".wscale") else self.dtype
            _require_cuda(t, name, want)
            _lib.check(self.lib.dk_mmdit_bind(self._h, name.encode(), t.data_ptr()), f"bind {name}")
        self.guidance = 3.5  # FLUX.1-dev's default distilled-guidance strength; only read when config.guidance_embed
        self._shape = None
        self._ws = None
        self._n_cached = 0
        self.block_cache = False
        self.reference_size = (0, 0)  # latent cells of the reference image (prepare(reference_size=...)); (0, 0): none
        self._ref_cached = False
        self.skip_layers, self.fork_rows = (), 0  # ``set_skip_layers``; ((), 0): off
        self.perturbed_attention = ()  # ``set_perturbed_attention``: the blocks; (): off (it shares ``fork_rows``: one of the two at a time)

    def __del__(self):
        if getattr(self, "_h", None):
            self.lib.dk_mmdit_destroy(self._h)
            self._h = None

    def set_skip_layers(self, blocks=None, fork_rows: int = 0) -> None:
        """dk_mmdit_set_skip_layers (skip-layer guidance, include/dk_hip.h): the last ``fork_rows`` batch rows of every later ``forward_tokens``
        become a copy of the first ``fork_rows`` that joins in front of double block min(``blocks``) and sits out the blocks named; their rows of
        ``tokens_in``, of ``text`` and of the cached context are never read, and the caller repeats the pooled rows for them.  ``(None, 0)``: off.
        Takes effect at the next forward; nothing is re-prepared.  ``forward_head`` / ``forward_tail`` / ``run_blocks`` are refused while set."""
        blocks = [] if blocks is None else [int(b) for b in blocks]
        arr = (C.c_int32 * len(blocks))(*blocks) if blocks else None
        _lib.check(self.lib.dk_mmdit_set_skip_layers(self._h, arr, len(blocks), int(fork_rows)), "dk_mmdit_set_skip_layers")
        self.skip_layers, self.fork_rows = tuple(sorted(blocks)), int(fork_rows)

    def set_perturbed_attention(self, blocks=None, fork_rows: int = 0) -> None:
        """dk_mmdit_set_perturbed_attention (perturbed-attention guidance, include/dk_hip.h): the last ``fork_rows`` batch rows of every later
        ``forward_tokens`` become a copy of the first ``fork_rows`` that joins in front of double block min(``blocks``); in the blocks named their
        image queries attend to the text keys and to their own key only (one identity-attention launch beside the plain one).  Their rows of
        ``tokens_in``, of ``text`` and of the cached context are never read, and the caller repeats the pooled rows for them.  ``(None, 0)``:
        off.  Takes effect at the next forward; nothing is re-prepared.  Refused while skip layers are set, and ``forward_head`` /
        ``forward_tail`` / ``run_blocks`` are refused while this is."""
        blocks = [] if blocks is None else [int(b) for b in blocks]
        arr = (C.c_int32 * len(blocks))(*blocks) if blocks else None
        _lib.check(self.lib.dk_mmdit_set_perturbed_attention(self._h, arr, len(blocks), int(fork_rows)), "dk_mmdit_set_perturbed_attention")
        if blocks or self.perturbed_attention:
            self.fork_rows = int(fork_rows)
        self.perturbed_attention = tuple(sorted(blocks))

    def _check_pitched_weights(self) -> None:
        """The engine reads the long-reduction weights at ``dk_weight_pitch`` elements per row (include/dk_hip.h); the C ABI
        binds bare pointers, so the layout the packer produced is checked here, where the shapes are still known."""
        h, r = self.config.hidden_size, self.config.mlp_ratio
        for name, t in self.weights.items():
            fp8 = name.endswith(".weight_fp8")
            base = name[:-len(".weight_fp8" if fp8 else ".weight")] if (fp8 or name.endswith(".weight")) else ""
            k = r * h if base.endswith(".mlp.fc2") else (1 + r) * h if base.endswith(".linear2") else 0
            pitch = (self.lib.dk_weight_pitch_fp8 if fp8 else self.lib.dk_weight_pitch)(k) if k else 0
            if k and t.shape[1] != pitch:
                raise _lib.DkHipError(f"{name}: {t.shape[1]} elements per row, the engine expects dk_weight_pitch({k}) = "
                                      f"{pitch} (was the weight packed under a different pitch_min_k?)")

    # -- shape / workspace ---------------------------------------------------------------
    def prepare(self, batch: int, latent_size: Sequence[int], text_len: int, n_timesteps: int,
                reference_size: Optional[Sequence[int]] = None) -> None:
        """``reference_size``: the (h, w) latent cells of a reference image (``cache_reference``), or None for no reference rows."""
        shape = (batch, int(latent_size[0]), int(latent_size[1]), text_len, n_timesteps)
        ref = (0, 0) if reference_size is None else (int(reference_size[0]), int(reference_size[1]))
        if ref != self.reference_size:
            _lib.check(self.lib.dk_mmdit_set_reference_grid(self._h, *ref), "dk_mmdit_set_reference_grid")
            self.reference_size = ref
            self._shape = None
            self._ref_cached = False
        if self._shape == shape:
            return
        self._check_pitched_weights()
        nbytes = self.lib.dk_mmdit_workspace_bytes(self._h, *shape)
        dev = next(iter(self.weights.values())).device
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(self.lib.dk_mmdit_prepare(self._h, *shape, self._ws.data_ptr(), self._ws.numel(), _stream()),
                   "dk_mmdit_prepare")
        self._shape = shape
        self._n_cached = 0
        self._ctx_cached = False
        self._ref_cached = False
        self._cond_cached = False
        self._ctrl_cached = False
        self._ip_cached = False
        self.control_taps = None  # (dk_mmdit_prepare switches taps off: their shape was the previous problem's)

    @property
    def batch(self):
        return self._shape[0]

    def tokens_shape(self):
        b, hl, wl, _, _ = self._shape
        p = self.config.patch_size
        return (b, (hl // p) * (wl // p), self.config.patch_dim)

    def mod_rows(self) -> int:
        return self.lib.dk_mmdit_mod_rows(self._h)

    def mod_offset(self, kind: int, index: int) -> int:
        return self.lib.dk_mmdit_mod_offset(self._h, kind, index)

    def score_bound(self, kind: int, index: int) -> float:
        """dk_mmdit_score_bound: the bound on |scale q.k| block ``index`` (kind 0 double, 2 single) hands its joint attention launch; 0: unknown"""
        return float(self.lib.dk_mmdit_score_bound(self._h, kind, index))

    # -- reference API ---------------------------------------------------------------------
    def cache_modulation_params(self, pooled_text_embeddings: Tensor, timesteps: Sequence[float], guidance_rows=None) -> None:
        """MMDiT.cache_modulation_params (mmdit.py:77-180); ``timesteps`` are host floats
        already rounded to the activation dtype (quirk Q1).
        ``guidance_rows`` (configurations with ``guidance_embed``; dk_mmdit_set_guidance_rows): one guidance strength per batch row in place of
        ``self.guidance`` for this table -- FlowEdit evaluates its source and target rows at different values.  None: the scalar, and a table
        cached without the keyword after one with it is the scalar's again."""
        if self._shape is None:
            raise _lib.DkHipError("prepare() must be called before cache_modulation_params()")
        pooled = pooled_text_embeddings.to(self.dtype).contiguous()
        _require_cuda(pooled, "pooled_text_embeddings")
        if pooled.shape != (self._shape[0], self.config.pooled_text_embed_dim):
            raise _lib.DkHipError(f"pooled_text_embeddings shape {tuple(pooled.shape)} != (batch, pooled_dim)")
        ts = [float(t) for t in timesteps]
        if guidance_rows is not None and not self.config.guidance_embed:
            raise _lib.DkHipError("guidance_rows needs a configuration with a guidance embedding (guidance_embed)")
        if self.config.guidance_embed:
            _lib.check(self.lib.dk_mmdit_set_guidance(self._h, float(self.guidance)), "dk_mmdit_set_guidance")
        if guidance_rows is not None:
            g = [float(v) for v in guidance_rows]
            if len(g) != self._shape[0]:
                raise _lib.DkHipError(f"guidance_rows holds {len(g)} values, the prepared batch has {self._shape[0]} rows")
            _lib.check(self.lib.dk_mmdit_set_guidance_rows(self._h, (C.c_float * len(g))(*g), len(g)), "dk_mmdit_set_guidance_rows")
            self._guidance_rows_set = True
        elif getattr(self, "_guidance_rows_set", False):  # (never set: the engine is not told, its calls are what they were)
            _lib.check(self.lib.dk_mmdit_set_guidance_rows(self._h, None, 0), "dk_mmdit_set_guidance_rows")
            self._guidance_rows_set = False
        arr = (C.c_float * len(ts))(*ts)
        _lib.check(self.lib.dk_mmdit_cache_modulation_params(self._h, pooled.data_ptr(), arr, len(ts), _stream()),
                   "dk_mmdit_cache_modulation_params")
        self._pooled_keepalive = pooled
        self._n_cached = len(ts)

    def clear_guidance_rows(self) -> None:
        """Back to the scalar ``self.guidance`` if ``cache_modulation_params(..., guidance_rows=...)`` set per-row values: the table must be cached
        again before the next forward.  Nothing is called on an engine that never had rows."""
        if getattr(self, "_guidance_rows_set", False):
            _lib.check(self.lib.dk_mmdit_set_guidance_rows(self._h, None, 0), "dk_mmdit_set_guidance_rows")
            self._guidance_rows_set = False
            self._n_cached = 0

    def cache_context(self, text: Tensor) -> None:
        """Step-invariant hoist of ``context_embedder(text)`` (mmdit.py:195): embedded once here, ``forward_tokens(..., None, i)``
        then reuses it in every step (the reference recomputes the same values per call)."""
        _require_cuda(text, "text", self.dtype)
        if tuple(text.shape) != (self._shape[0], self._shape[3], self.config.token_level_text_embed_dim):
            raise _lib.DkHipError(f"text shape {tuple(text.shape)} does not match the prepared problem")
        _lib.check(self.lib.dk_mmdit_cache_context(self._h, text.data_ptr(), _stream()), "dk_mmdit_cache_context")
        self._ctx_cached = True

    def reference_tokens(self) -> int:
        """S_r: rows of the reference image behind the image rows of every batch row (0 without one)."""
        p = self.config.patch_size
        return (self.reference_size[0] // p) * (self.reference_size[1] // p)

    def cache_reference(self, latent_or_tokens: Tensor, per_image: bool = False) -> None:
        """Reference-image conditioning (FLUX.1 Kontext's token layout, include/dk_hip.h): embeds the reference once; every later
        forward carries its rows behind the image rows.  ``latent_or_tokens``: the reference latent, f32 NHWC [n, rh, rw, C] with
        (rh, rw) the ``reference_size`` given to ``prepare``, or its tokens in the engine's dtype [n, S_r, p*p*C]; n = batch with
        ``per_image``, else 1 (one reference for every batch row)."""
        if self._shape is None or self.reference_size == (0, 0):
            raise _lib.DkHipError("cache_reference() needs prepare(..., reference_size=(h, w)) first")
        t = latent_or_tokens
        if t.dim() == 4:
            if tuple(t.shape[1:3]) != self.reference_size:
                raise _lib.DkHipError(f"reference latent {tuple(t.shape[1:3])} != the prepared reference_size {self.reference_size}")
            t = self.patchify(t.to(torch.float32).contiguous())
        _require_cuda(t, "reference tokens", self.dtype)
        want = (self._shape[0] if per_image else 1, self.reference_tokens(), self.config.patch_dim)
        if tuple(t.shape) != want:
            raise _lib.DkHipError(f"reference tokens shape {tuple(t.shape)} != {want}")
        _lib.check(self.lib.dk_mmdit_cache_reference(self._h, t.data_ptr(), int(bool(per_image)), _stream()), "dk_mmdit_cache_reference")
        self._ref_cached = True

    def cache_condition(self, tokens: Tensor, per_image: bool = False) -> None:
        """Channel-concatenated conditioning (FLUX.1 Fill / Canny / Depth, include/dk_hip.h): the condition token rows
        (``ops.fill_condition_tokens``), bf16 [n, S_i, condition_features]; n = batch with ``per_image``, else 1 (one condition for every
        batch row).  Their share of x_embedder is computed once here and added in every later forward."""
        if self._shape is None or not self.condition_features:
            raise _lib.DkHipError("cache_condition() needs a configuration with condition_features > 0 and prepare() first")
        _require_cuda(tokens, "condition tokens", self.dtype)
        want = (self._shape[0] if per_image else 1, self.tokens_shape()[1], self.condition_features)
        if tuple(tokens.shape) != want:
            raise _lib.DkHipError(f"condition tokens shape {tuple(tokens.shape)} != {want}")
        _lib.check(self.lib.dk_mmdit_cache_condition(self._h, tokens.data_ptr(), int(bool(per_image)), _stream()), "dk_mmdit_cache_condition")
        self._cond_cached = True

    # -- SD3 ControlNet (include/dk_hip.h; no reference counterpart) ---------------------------------------------------------
    def taps_shape(self):
        """[N_c, batch, S_i, h]: what ``control_forward`` of this (control-net) engine writes."""
        b, s_i, _ = self.tokens_shape()
        n = self.config.depth_multimodal + (self.config.depth_unified if self.control_net_flux else 0)  # (FLUX: the double blocks' taps first)
        return (n, b, s_i, self.config.hidden_size)

    def cache_control_image(self, latent_or_tokens: Tensor, per_image: bool = False) -> None:
        """dk_mmdit_cache_control_image: the VAE-encoded control image, f32 NHWC latent [n, Hl, Wl, C] of the prepared size or its tokens in the
        engine's dtype [n, S_i, p*p*C]; n = batch with ``per_image``, else 1 (one control image for every batch row).  Its share of the patch
        embedding (with the positional rows) is computed once here and added in every later ``control_forward``."""
        if self._shape is None or not self.control_net:
            raise _lib.DkHipError("cache_control_image() needs a configuration with control_net = True and prepare() first")
        t = latent_or_tokens
        if t.dim() == 4:
            if tuple(t.shape[1:3]) != tuple(self._shape[1:3]):
                raise _lib.DkHipError(f"control latent {tuple(t.shape[1:3])} != the prepared latent size {tuple(self._shape[1:3])}")
            t = self.patchify(t.to(torch.float32).contiguous())
        _require_cuda(t, "control tokens", self.dtype)
        want = (self._shape[0] if per_image else 1,) + self.tokens_shape()[1:]
        if tuple(t.shape) != want:
            raise _lib.DkHipError(f"control tokens shape {tuple(t.shape)} != {want}")
        _lib.check(self.lib.dk_mmdit_cache_control_image(self._h, t.data_ptr(), int(bool(per_image)), _stream()), "dk_mmdit_cache_control_image")
        self._ctrl_cached = True

    def control_forward(self, tokens_in: Tensor, text: Optional[Tensor], step_index: int, taps_out: Optional[Tensor] = None) -> Tensor:
        """dk_mmdit_control_forward: the ControlNet on ``tokens_in`` (the main model's tokens of this evaluation) -> taps [N_c, batch, S_i, h]
        for the main engine's ``set_control_taps``.  ``text=None`` uses ``cache_context``'s result."""
        if not self.control_net:
            raise _lib.DkHipError("control_forward() needs a configuration with control_net = True")
        self._check_forward_args(tokens_in, text, step_index)
        if not self._ctrl_cached:
            raise _lib.DkHipError("control_forward() needs cache_control_image() after prepare()")
        if taps_out is None:
            taps_out = torch.empty(self.taps_shape(), dtype=self.dtype, device=tokens_in.device)
        _require_cuda(taps_out, "taps_out", self.dtype)
        if tuple(taps_out.shape) != self.taps_shape():
            raise _lib.DkHipError(f"taps_out shape {tuple(taps_out.shape)} != {self.taps_shape()}")
        _lib.check(self.lib.dk_mmdit_control_forward(self._h, tokens_in.data_ptr(), None if text is None else text.data_ptr(), step_index,
                                                     taps_out.data_ptr(), _stream()), "dk_mmdit_control_forward")
        return taps_out

    def set_control_taps(self, taps: Optional[Tensor] = None, scale: float = 1.0) -> None:
        """dk_mmdit_set_control_taps on the MAIN engine: every later ``forward_tokens`` adds ``scale * taps[floor(g * n / depth)]`` to the image
        stream behind block g (g < depth - 1), inside the next block's first LayerNorm launch.  ``taps``: [n, batch, S_i, h] in the engine's
        dtype, read in stream order at every forward (the caller may rewrite it between forwards); None: off.  Nothing is re-prepared.
        ``forward_head`` / ``forward_tail`` / ``run_blocks`` are refused while set."""
        if taps is None:
            _lib.check(self.lib.dk_mmdit_set_control_taps(self._h, None, 0, 0.0), "dk_mmdit_set_control_taps")
            self.control_taps = None
            return
        if self._shape is None:
            raise _lib.DkHipError("set_control_taps() needs prepare() first: the taps' shape is the prepared problem's")
        _require_cuda(taps, "taps", self.dtype)
        b, s_i, _ = self.tokens_shape()
        if taps.dim() != 4 or tuple(taps.shape[1:]) != (b, s_i, self.config.hidden_size):
            raise _lib.DkHipError(f"taps shape {tuple(taps.shape)} != (n, {b}, {s_i}, {self.config.hidden_size})")
        _lib.check(self.lib.dk_mmdit_set_control_taps(self._h, taps.data_ptr(), int(taps.shape[0]), float(scale)), "dk_mmdit_set_control_taps")
        self.control_taps = (taps, float(scale))

    def set_flux_control_taps(self, taps: Optional[Tensor] = None, n_double_taps: int = 0, scale: float = 1.0) -> None:
        """dk_mmdit_set_flux_control_taps on the MAIN engine (FLUX family, bf16): ``taps`` [n_double_taps + n_single_taps, batch, S_i, h], the
        double blocks' taps first -- what a FLUX control-net engine's ``control_forward`` writes, with ``n_double_taps`` its ``depth_multimodal``.
        Every later ``forward_tokens`` adds ``scale * tap[g // ceil(depth / n)]`` (per kind; diffusers' FluxTransformer2DModel rule) to the image
        rows behind block g, the last block of each kind included, inside the LayerNorm launch that reads those rows next.  None: off.  Nothing
        is re-prepared.  ``forward_head`` / ``forward_tail`` / ``run_blocks`` are refused while set."""
        if taps is None:
            _lib.check(self.lib.dk_mmdit_set_flux_control_taps(self._h, None, 0, 0, 0.0), "dk_mmdit_set_flux_control_taps")
            self.control_taps = None
            return
        if self._shape is None:
            raise _lib.DkHipError("set_flux_control_taps() needs prepare() first: the taps' shape is the prepared problem's")
        _require_cuda(taps, "taps", self.dtype)
        b, s_i, _ = self.tokens_shape()
        if taps.dim() != 4 or tuple(taps.shape[1:]) != (b, s_i, self.config.hidden_size):
            raise _lib.DkHipError(f"taps shape {tuple(taps.shape)} != (n, {b}, {s_i}, {self.config.hidden_size})")
        n_double_taps = int(n_double_taps)
        if not 0 <= n_double_taps <= taps.shape[0]:
            raise _lib.DkHipError(f"n_double_taps = {n_double_taps}: must lie in [0, {taps.shape[0]}], the number of taps")
        _lib.check(self.lib.dk_mmdit_set_flux_control_taps(self._h, taps.data_ptr(), n_double_taps, int(taps.shape[0]) - n_double_taps, float(scale)),
                   "dk_mmdit_set_flux_control_taps")
        self.control_taps = (taps, float(scale))

    # -- FLUX IP-Adapter (include/dk_hip.h; no reference counterpart) ----------------------------------------------------------
    def ip_tokens_shape(self, per_image: bool = True):
        return (self._shape[0] if per_image else 1, self.ip_adapter.ip_adapter_tokens, self.ip_adapter.ip_adapter_dim)

    def cache_ip_tokens(self, tokens: Tensor, per_image: bool = False) -> None:
        """dk_mmdit_cache_ip_tokens: the image prompt's tokens (``ip_adapter_project``), bf16 [n, N, C]; n = batch with ``per_image``, else 1 (one
        prompt for every batch row).  Every double block's keys and values are computed once here; a later call replaces them."""
        if self._shape is None or self.ip_adapter is None:
            raise _lib.DkHipError("cache_ip_tokens() needs an engine built with ip_adapter= and prepare() first")
        _require_cuda(tokens, "image-prompt tokens", self.dtype)
        if tuple(tokens.shape) != self.ip_tokens_shape(per_image):
            raise _lib.DkHipError(f"image-prompt tokens shape {tuple(tokens.shape)} != {self.ip_tokens_shape(per_image)}")
        _lib.check(self.lib.dk_mmdit_cache_ip_tokens(self._h, tokens.data_ptr(), int(bool(per_image)), _stream()), "dk_mmdit_cache_ip_tokens")
        self._ip_cached = True

    def set_ip_scale(self, scale: float = 0.0) -> None:
        """dk_mmdit_set_ip_scale: 0 is off (the plain launches and their bits); with another scale every later ``forward_tokens`` adds
        ``scale * ip_i`` to the image stream behind double block i.  ``forward_head`` / ``forward_tail`` / ``run_blocks`` are refused while on."""
        _lib.check(self.lib.dk_mmdit_set_ip_scale(self._h, float(scale)), "dk_mmdit_set_ip_scale")
        self.ip_scale = float(scale)

    def forward_tokens(self, tokens_in: Tensor, text: Optional[Tensor], step_index: int, tokens_out: Optional[Tensor] = None) -> Tensor:
        """MMDiT.__call__ between patchify and unpatchify (mmdit.py:188-252).  ``text=None`` uses ``cache_context``'s result."""
        self._check_forward_args(tokens_in, text, step_index)
        if tokens_out is None:
            tokens_out = torch.empty_like(tokens_in)
        _lib.check(self.lib.dk_mmdit_forward(self._h, tokens_in.data_ptr(), None if text is None else text.data_ptr(), step_index,
                                             tokens_out.data_ptr(), _stream()), "dk_mmdit_forward")
        return tokens_out

    def _check_forward_args(self, tokens_in: Tensor, text: Optional[Tensor], step_index: int) -> None:
        _require_cuda(tokens_in, "tokens_in", self.dtype)
        if tuple(tokens_in.shape) != self.tokens_shape():
            raise _lib.DkHipError(f"tokens_in shape {tuple(tokens_in.shape)} != {self.tokens_shape()}")
        if text is None:
            if not getattr(self, "_ctx_cached", False):
                raise _lib.DkHipError("forward_tokens(text=None) needs cache_context(text) after prepare()")
        else:
            _require_cuda(text, "text", self.dtype)
            if tuple(text.shape) != (self._shape[0], self._shape[3], self.config.token_level_text_embed_dim):
                raise _lib.DkHipError(f"text shape {tuple(text.shape)} does not match the prepared problem")
        if not (0 <= step_index < self._n_cached):
            raise KeyError(f"no cached modulation parameters for step {step_index}")  # reference: dict KeyError

    # -- first-block cache (include/dk_hip.h; no reference counterpart) ----------------------------------------------------
    def enable_block_cache(self, on: bool = True) -> None:
        """Turn the first-block cache on or off.  The workspace layout changes with it, so the next ``prepare`` carves again (and the
        modulation parameters and the context must be cached again)."""
        if bool(on) == self.block_cache:
            return
        _lib.check(self.lib.dk_mmdit_set_block_cache(self._h, int(bool(on))), "dk_mmdit_set_block_cache")
        self.block_cache = bool(on)
        self._shape = None
        self._n_cached = 0
        self._ctx_cached = False

    def reset_block_cache(self) -> None:
        _lib.check(self.lib.dk_mmdit_reset_block_cache(self._h), "dk_mmdit_reset_block_cache")

    def forward_head(self, tokens_in: Tensor, text: Optional[Tensor], step_index: int) -> Tensor:
        """Embedders, block 0 and the probe of step ``step_index``: returns f32 [batch, 2] on the device, (num, den) per batch row =
        (sum |D_cur - D_ref|, sum |D_ref|) over the image rows (den = 0 before any computed step).  Nothing synchronises: read it
        (``.cpu()``) to decide, then call ``forward_tail`` for the same step."""
        self._check_forward_args(tokens_in, text, step_index)
        probe = torch.empty(self._shape[0], 2, dtype=torch.float32, device=tokens_in.device)
        _lib.check(self.lib.dk_mmdit_forward_head(self._h, tokens_in.data_ptr(), None if text is None else text.data_ptr(), step_index,
                                                  probe.data_ptr(), _stream()), "dk_mmdit_forward_head")
        return probe

    def forward_tail(self, step_index: int, reuse: bool, tokens_out: Optional[Tensor] = None) -> Tensor:
        """The rest of the step whose head ran last.  ``reuse`` False: blocks 1 .. L-1 and the final layer, and their effect on the
        image rows is cached; True: that cached effect is added instead and only the final layer runs."""
        if self._shape is None:
            raise _lib.DkHipError("prepare() must be called before forward_tail()")
        if tokens_out is None:
            tokens_out = torch.empty(self.tokens_shape(), dtype=self.dtype, device=self._ws.device)
        _require_cuda(tokens_out, "tokens_out", self.dtype)
        if tuple(tokens_out.shape) != self.tokens_shape():
            raise _lib.DkHipError(f"tokens_out shape {tuple(tokens_out.shape)} != {self.tokens_shape()}")
        _lib.check(self.lib.dk_mmdit_forward_tail(self._h, step_index, int(bool(reuse)), tokens_out.data_ptr(), _stream()),
                   "dk_mmdit_forward_tail")
        return tokens_out

    def run_blocks(self, x: Tensor, step_index: int, first_block: int, n_blocks: int = 1) -> Tensor:
        """MultiModalTransformerBlock / UnifiedTransformerBlock.__call__ (mmdit.py:568-675, 693-751) on a caller-supplied joint
        residual stream ``x`` (bf16 [batch, S_t + S_i (+ S_r), h], text rows first): blocks ``first_block .. first_block + n_blocks - 1`` of
        the global order (double blocks, then single blocks) with the modulation cached for ``step_index``."""
        _require_cuda(x, "x", self.dtype)
        b, hl, wl, s_t, _ = self._shape
        p = self.config.patch_size
        want = (b, s_t + (hl // p) * (wl // p) + self.reference_tokens(), self.config.hidden_size)
        if tuple(x.shape) != want:
            raise _lib.DkHipError(f"x shape {tuple(x.shape)} != {want}")
        if not (0 <= step_index < self._n_cached):
            raise KeyError(f"no cached modulation parameters for step {step_index}")
        out = torch.empty_like(x)
        _lib.check(self.lib.dk_mmdit_run_blocks(self._h, x.data_ptr(), out.data_ptr(), step_index, first_block, n_blocks, _stream()),
                   "dk_mmdit_run_blocks")
        return out

    def patchify(self, latent: Tensor, dup: int = 1) -> Tensor:
        """LatentImageAdapter reshape (mmdit.py:292-300): f32 NHWC -> bf16 tokens."""
        _require_cuda(latent, "latent", torch.float32)
        n, hl, wl, c = latent.shape
        p = self.config.patch_size
        tok = torch.empty(n * dup, (hl // p) * (wl // p), p * p * c, dtype=self.dtype, device=latent.device)
        fn = self.lib.dk_latent_to_tokens_f16 if self.dtype == torch.float16 else self.lib.dk_latent_to_tokens
        _lib.check(fn(latent.data_ptr(), tok.data_ptr(), n, dup, hl, wl, c, p,
                                                int(self.config.patchify_via_reshape), _stream()), "dk_latent_to_tokens")
        return tok

    def __call__(self, latent_image_embeddings: Tensor, token_level_text_embeddings: Tensor, step_index: int) -> Tensor:
        """MMDiT.__call__ (mmdit.py:188-266) for NHWC latents; returns tokens-major FinalLayer
        output un-patchified to NHWC bf16 (used by parity tests; the step loop stays fused)."""
        lat = latent_image_embeddings.to(torch.float32).contiguous()
        tok = self.patchify(lat)
        text = token_level_text_embeddings
        if text.dim() == 4:  # reference passes [B, S_t, 1, T]
            text = text.squeeze(2)
        out = self.forward_tokens(tok, text.to(self.dtype).contiguous(), step_index)
        return unpatchify_tokens(out, self.config, lat.shape[1], lat.shape[2])


def ip_adapter_project(weights: Dict[str, Tensor], ip, image_embeds: Tensor) -> Tensor:
    """The IP-Adapter's projection model, once per call, as torch ops on the device: tok = LayerNorm_C(reshape(Linear(E -> N C)(e), [N, C])), affine,
    rounded to bf16 behind the Linear and behind the norm.  image_embeds: [n, E] -> bf16 [n, N, C] for ``MMDiTEngine.cache_ip_tokens``."""
    N, Cd = ip.ip_adapter_tokens, ip.ip_adapter_dim
    w = weights["ip_adapter.proj.weight"]
    e = image_embeds.to(device=w.device, dtype=torch.bfloat16)
    if e.dim() != 2 or e.shape[1] != ip.embed_dim:
        raise _lib.DkHipError(f"image embeddings shape {tuple(image_embeds.shape)} != (n, {ip.embed_dim})")
    y = torch.nn.functional.linear(e.float(), w.float(), weights["ip_adapter.proj.bias"].float()).to(torch.bfloat16).reshape(e.shape[0], N, Cd)
    y = torch.nn.functional.layer_norm(y.float(), (Cd,), weights["ip_adapter.norm.weight"].float(), weights["ip_adapter.norm.bias"].float(), ip.norm_eps)
    return y.to(torch.bfloat16).contiguous()


def unpatchify_tokens(tok: Tensor, cfg: MMDiTConfig, hl: int, wl: int) -> Tensor:
    """Pure index shuffle used only by tests / the NHWC convenience call
    (mmdit.py:304-321, 975-988); the production step loop does this inside dk_euler_cfg_step."""
    b = tok.shape[0]
    p, c = cfg.patch_size, cfg.vae_latent_dim
    h, w = hl // p, wl // p
    if cfg.patchify_via_reshape:
        return tok.reshape(b, h, w, c, p, p).permute(0, 1, 4, 2, 5, 3).reshape(b, hl, wl, c)
    return tok.reshape(b, h, w, p, p, c).permute(0, 1, 3, 2, 4, 5).reshape(b, hl, wl, c)


def _vae_set_dtype(lib, handle, config):
    """element type of a VAE half from ``config.dtype`` ("bfloat16" default | "float16"), set on the handle before the first bind: the torch dtype
    every bound tensor, ``raw`` (decoder) and the moments (encoder) then have"""
    name = getattr(config, "dtype", "bfloat16")
    if name not in _ACT_DTYPE:
        raise _lib.DkHipError(f"unknown VAE dtype {name!r} (bfloat16 | float16)")
    code, dt = _ACT_DTYPE[name]
    _lib.check(lib.dk_vae_set_dtype(handle, code), "dk_vae_set_dtype")
    return dt


class VAEDecoderEngine:
    """Drop-in for the reference ``VAEDecoder`` (+ the clip / uint8 tail).  ``config.dtype`` "float16": fp16 weights, activations and ``raw``
    (the reference's decoder dtype for SD3); bf16 tensors are then refused."""

    def __init__(self, config: VAEDecoderConfig, packed_weights: Dict[str, Tensor]):
        self.lib = _lib.load()
        self.config = config
        c = _lib.dk_vae_config()
        c.in_channels, c.out_channels = config.in_channels, config.out_channels
        for i, ch in enumerate(config.block_out_channels):
            c.block_out_channels[i] = ch
        c.n_blocks = len(config.block_out_channels)
        c.layers_per_block, c.resnet_groups = config.layers_per_block, config.resnet_groups
        c.group_norm_eps = config.group_norm_eps
        h = C.c_void_p()
        _lib.check(self.lib.dk_vae_create(C.byref(c), C.byref(h)), "dk_vae_create")
        self._h = h
        self.dtype = _vae_set_dtype(self.lib, h, config)
        self.weights = packed_weights
        for name, t in packed_weights.items():
            _require_cuda(t, name, self.dtype)
            _lib.check(self.lib.dk_vae_bind(self._h, name.encode(), t.data_ptr()), f"bind {name}")
        self._ws = None

    def __del__(self):
        if getattr(self, "_h", None):
            self.lib.dk_vae_destroy(self._h)
            self._h = None

    def decode(self, x: Tensor, want_raw: bool = False):
        """x: f32 [B,h,w,16] -> (image f32 [B,8h,8w,3] in [0,1], uint8 image, raw in ``self.dtype`` or None)."""
        x = x.to(torch.float32).contiguous()
        _require_cuda(x, "latent")
        b, h, w, _ = x.shape
        nbytes = self.lib.dk_vae_workspace_bytes(self._h, b, h, w)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        scale = 2 ** (len(self.config.block_out_channels) - 1)
        img = torch.empty(b, h * scale, w * scale, 3, dtype=torch.float32, device=x.device)
        u8 = torch.empty(b, h * scale, w * scale, 3, dtype=torch.uint8, device=x.device)
        raw = torch.empty(b, h * scale, w * scale, 4, dtype=self.dtype, device=x.device) if want_raw else None
        _lib.check(self.lib.dk_vae_decode(self._h, x.data_ptr(), b, h, w, img.data_ptr(), u8.data_ptr(), _ptr(raw),
                                          self._ws.data_ptr(), self._ws.numel(), _stream()), "dk_vae_decode")
        return img, u8, raw

    def __call__(self, x: Tensor) -> Tensor:
        """VAEDecoder.__call__ (vae.py:386-401): returns the un-clipped decoder output [B,8h,8w,3]."""
        _, _, raw = self.decode(x, want_raw=True)
        return raw[..., :3]


class VAEEncoderEngine:
    """Drop-in for the reference ``VAEEncoder`` (vae.py:404-467): image in [-1, 1] -> moments.  ``config.dtype`` "float16": fp16 weights,
    activations and moments (the reference runs its encoder in fp32: fp16 is the closer 16-bit form, not its dtype)."""

    def __init__(self, config, packed_weights: Dict[str, Tensor]):
        self.lib = _lib.load()
        self.config = config
        c = _lib.dk_vae_config()
        c.in_channels, c.out_channels = config.in_channels, config.out_channels
        for i, ch in enumerate(config.block_out_channels):
            c.block_out_channels[i] = ch
        c.n_blocks = len(config.block_out_channels)
        c.layers_per_block, c.resnet_groups = config.layers_per_block, config.resnet_groups
        c.group_norm_eps = config.group_norm_eps
        h = C.c_void_p()
        _lib.check(self.lib.dk_vae_create(C.byref(c), C.byref(h)), "dk_vae_create")
        self._h = h
        self.dtype = _vae_set_dtype(self.lib, h, config)
        self.weights = packed_weights
        for name, t in packed_weights.items():
            _require_cuda(t, name, self.dtype)
            _lib.check(self.lib.dk_vae_bind(self._h, name.encode(), t.data_ptr()), f"bind {name}")
        self._ws = None

    def __del__(self):
        if getattr(self, "_h", None):
            self.lib.dk_vae_destroy(self._h)
            self._h = None

    def encode(self, image: Tensor):
        """image: f32 [B,H,W,3] in [-1,1] -> moments in ``self.dtype`` [B,H/8,W/8,ldm] (mean | logvar in the first
        ``out_channels`` columns)."""
        image = image.to(torch.float32).contiguous()
        _require_cuda(image, "image")
        b, H, W, _ = image.shape
        nbytes = self.lib.dk_vae_encoder_workspace_bytes(self._h, b, H, W)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=image.device)
        down = 2 ** (len(self.config.block_out_channels) - 1)
        ldm = (self.config.out_channels + 3) // 4 * 4
        mom = torch.empty(b, H // down, W // down, ldm, dtype=self.dtype, device=image.device)
        _lib.check(self.lib.dk_vae_encode(self._h, image.data_ptr(), b, H, W, mom.data_ptr(), ldm, None,
                                          self._ws.data_ptr(), self._ws.numel(), _stream()), "dk_vae_encode")
        return mom

    def __call__(self, image: Tensor) -> Tensor:
        """VAEEncoder.__call__ (vae.py:456-467): hidden [B,H/8,W/8,out_channels]."""
        return self.encode(image)[..., :self.config.out_channels]

    def sample(self, moments: Tensor, noise: Tensor) -> Tensor:
        """encode_image_to_latents tail (__init__.py:588-594): mean + exp(0.5 * clip(logvar)) * noise, f32."""
        _require_cuda(moments, "moments", self.dtype)
        noise = noise.to(torch.float32).contiguous()
        _require_cuda(noise, "noise")
        L = self.config.out_channels // 2
        b, h, w, ldm = moments.shape
        assert noise.shape == (b, h, w, L), (noise.shape, (b, h, w, L))
        out = torch.empty(b, h, w, L, dtype=torch.float32, device=moments.device)
        name = "dk_latent_sample_f16" if self.dtype == torch.float16 else "dk_latent_sample_f32"
        _lib.check(getattr(self.lib, name)(moments.data_ptr(), ldm, noise.data_ptr(), out.data_ptr(), b * h * w, L, _stream()), name)
        return out
