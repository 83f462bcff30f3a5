"""FLUX ControlNet for the parity tests: the CPU oracles of the ControlNet (diffusers' FluxControlNetModel layout) and of a main model that takes
its double- and single-block taps, and a writer of the diffusers checkpoint layout.

Both oracles extend ``oracle.mmdit.OracleMMDiT`` -- the restatement pinned against the reference -- by what the reference lacks, from the
published model definition (diffusers' FluxControlNetModel.forward and FluxTransformer2DModel.forward):

  * ``FluxControlNetOracle``: the embedders, ``controlnet_x_embedder`` on the packed control latent, every double block with
    ``controlnet_blocks.j`` on the image stream behind it, every single block with ``controlnet_single_blocks.j`` on the image rows of the joint
    stream behind it.  Taps: [n_double + n_single, B, S_i, h], the double blocks' first.
  * ``ControlledFluxOracle``: ``round(x + s * tap[g // ceil(depth / n)])`` on the image rows behind EVERY double and every single block, per kind
    (diffusers' index rule for FLUX: not the SD3 one).  The scalar s is fp32.

Rounding points follow the base class (one per Linear output, modulate, norm and gated add) and the engine's association of the two patch
embeddings:  image rows = round( round(x_embedder(tokens)) + round(controlnet_x_embedder(control tokens)) )  -- the control image's share is
computed and rounded once per call (dk_mmdit_cache_control_image) and added in the x_embedder launch's residual epilogue.  The published code
rounds s * tap and the sum separately; here the add is one rounding (include/dk_hip.h).

The joint attention of a double block runs in FLUX order, [text, image], whatever ``depth_unified`` is: the base class switches to the SD3 order
for a model without single blocks, whose RoPE table (text positions first) it would then apply to the wrong rows.  Attention does not depend on
the order of its keys, so with the table on the right rows this is the function the engine computes for depth_unified == 0 as well.

Arithmetic restatement only: no ControlNet checkpoint has been run."""
import math

import torch

from oracle.mmdit import OracleMMDiT, linear, rope_apply, rope_table, sdpa
from tests._controlnet import ChainOracle, evaluations_active  # noqa: F401  (reused as they are: the chain calls cn(latent, text, t, control))


def flux_tap_index(g: int, n_taps: int, depth: int) -> int:
    """the tap added behind block g of a kind with ``depth`` blocks and ``n_taps`` taps: diffusers' g // int(np.ceil(depth / n_taps)) in integers"""
    return g // ((depth + n_taps - 1) // n_taps)


def sd3_tap_index(g: int, n_taps: int, depth: int) -> int:
    return g * n_taps // depth


class _FluxOrder(OracleMMDiT):
    def _double_block(self, i, img, txt, tkey, rope):
        cfg, P = self.cfg, self.P
        pi = f"multimodal_transformer_blocks.{i}.image_transformer_block"
        pt = f"multimodal_transformer_blocks.{i}.text_transformer_block"
        skip_txt = (i == cfg.depth_multimodal - 1) and cfg.depth_unified < 1
        ii = self._pre_sdpa(img, pi, tkey, 6)
        ti = self._pre_sdpa(txt, pt, tkey, 2 if skip_txt else 6)
        S_t = txt.shape[1]
        q, k, v = (torch.cat([ti[n], ii[n]], dim=2) for n in "qkv")
        if rope is not None:
            q, k = rope_apply(q, rope, P), rope_apply(k, rope, P)
        o = self._merge(sdpa(q, k, v, 1.0 / math.sqrt(cfg.head_dim), P))
        img = self._post_sdpa(img, o[:, S_t:], ii, pi, False)
        txt = None if skip_txt else self._post_sdpa(txt, o[:, :S_t], ti, pt, False)
        return img, txt

    def _rope_for(self, S_t, Hl, Wl):
        cfg = self.cfg
        key = (S_t, Hl // cfg.patch_size, Wl // cfg.patch_size)
        if self._rope_key != key:
            self._rope, self._rope_key = rope_table(cfg, *key), key
        return self._rope

    def _tokens(self, x):
        cfg = self.cfg
        B, Hl, Wl, C = x.shape
        p = cfg.patch_size
        assert cfg.patchify_via_reshape
        return x.reshape(B, Hl // p, p, Wl // p, p, C).permute(0, 1, 3, 5, 2, 4).reshape(B, (Hl // p) * (Wl // p), -1)


class FluxControlNetOracle(_FluxOrder):
    def _adaln_names(self):
        return [n for n in super()._adaln_names() if n != "final_layer"]

    def __call__(self, latent, text, timestep, control_latent, taps=None):
        """-> [n_double + n_single, B, S_i, h]; ``control_latent``: [B or 1, Hl, Wl, C], already in the latent format.  ``taps``: optional dict
        that receives the streams (embed_img, embed_txt, double{i}_img, double{i}_txt, single{i}) as OracleMMDiT's does."""
        cfg, P = self.cfg, self.P
        tkey = float(timestep)
        B, Hl, Wl, _ = latent.shape
        txt = self._lin(P.r(text), "context_embedder")
        wx, wc = self.w["x_embedder.proj.weight"], self.w["controlnet_x_embedder.proj.weight"]
        conde = linear(self._tokens(P.r(control_latent)), wc.reshape(wc.shape[0], -1), self.w["controlnet_x_embedder.proj.bias"], P).expand(B, -1, -1)
        img = P.r(linear(self._tokens(P.r(latent)), wx.reshape(wx.shape[0], -1), self.w["x_embedder.proj.bias"], P) + conde)
        rope = self._rope_for(txt.shape[1], Hl, Wl)
        if taps is not None:
            taps["embed_img"], taps["embed_txt"] = img.clone(), txt.clone()
        out = []
        for i in range(cfg.depth_multimodal):
            img, txt = self._double_block(i, img, txt, tkey, rope)
            if taps is not None:
                taps[f"double{i}_img"] = img.clone()
                if txt is not None:
                    taps[f"double{i}_txt"] = txt.clone()
            out.append(self._lin(img, f"controlnet_blocks.{i}"))
        if cfg.depth_unified > 0:
            S_t = txt.shape[1]
            x = torch.cat([txt, img], dim=1)
            for i in range(cfg.depth_unified):
                x = self._single_block(i, x, tkey, rope)
                if taps is not None:
                    taps[f"single{i}"] = x.clone()
                out.append(self._lin(x[:, S_t:], f"controlnet_single_blocks.{i}"))
        return torch.stack(out)


class ControlledFluxOracle(_FluxOrder):
    """``control`` = (taps [n_double_taps + n_single_taps, B, S_i, h], n_double_taps, scale) or None; set it before a call"""
    control = None

    def _scale(self):
        return float(torch.tensor(self.control[2], dtype=torch.float32))  # (the engine's scalar is fp32)

    def _double_block(self, i, img, txt, tkey, rope):
        img, txt = super()._double_block(i, img, txt, tkey, rope)
        if self.control is not None and self.control[1] > 0:
            taps, nd = self.control[0], self.control[1]
            img = self.P.r(img + self._scale() * taps[flux_tap_index(i, nd, self.cfg.depth_multimodal)])
        return img, txt

    def _single_block(self, i, x, tkey, rope):
        x = super()._single_block(i, x, tkey, rope)
        if self.control is not None and self.control[0].shape[0] > self.control[1]:
            taps, nd = self.control[0], self.control[1]
            S_t = x.shape[1] - taps.shape[2]
            tap = taps[nd + flux_tap_index(i, taps.shape[0] - nd, self.cfg.depth_unified)]
            x = torch.cat([x[:, :S_t], self.P.r(x[:, S_t:] + self._scale() * tap)], dim=1)
        return x

    def __call__(self, latent, text, timestep, taps=None):
        if self.cfg.depth_unified > 0:
            return super().__call__(latent, text, timestep, taps)
        # (the base class builds no RoPE-ordered joint stream without single blocks: the same forward with the table of this class's order)
        cfg, P = self.cfg, self.P
        tkey = float(timestep)
        B, Hl, Wl, _ = latent.shape
        txt = self._lin(P.r(text), "context_embedder")
        img = self._patch_embed(P.r(latent))
        rope = self._rope_for(txt.shape[1], Hl, Wl)
        for i in range(cfg.depth_multimodal):
            img, txt = self._double_block(i, img, txt, tkey, rope)
        mod = self._mod["final_layer"][tkey].chunk(2, dim=-1)
        from oracle.mmdit import affine_transform
        y = self._lin(affine_transform(img, mod[0], mod[1], cfg.layer_norm_eps, P), "final_layer.linear")
        if taps is not None:
            taps["final"] = y.clone()
        return self._unpatch(y, Hl, Wl)


class FluxChainOracle(ChainOracle):
    """``ChainOracle`` with the FLUX form of the main oracle's ``control``: every tap the ControlNet writes, its double blocks' first"""

    def __call__(self, latent, text, timestep):
        on = True if self.active is None else self.active[self.calls]
        self.calls += 1
        self.main.control = (self.cn(latent, text, timestep, self.control_latent), self.cn.cfg.depth_multimodal, self.scale) if on else None
        return self.main(latent, text, timestep)


# the synthetic taps of the main-engine tests and of the sensitivity condition (tests/test_flux_controlnet_cpu.py): N(0, TAP_STD^2) rounded to
# bf16, added under TAP_SCALE.  The pair is chosen so that zeroing any ONE of seven taps of the (4 double, 3 single) tiny model moves the fp32
# oracle's output by at least 10 x the gate's absolute term -- asserted there, not measured here
TAP_STD, TAP_SCALE = 0.03, 0.7


def synthetic_taps(n, B, S_i, h, seed=11):
    from tests._util import randn
    return randn(n, B, S_i, h, seed=seed, scale=TAP_STD)


def to_diffusers_flux_controlnet(w, cfg):
    """Reference-named FLUX ControlNet weights (synth_mmdit_weights of a ``control_net_flux`` config) -> the diffusers FluxControlNetModel layout
    ``flux_controlnet_checkpoint_to_reference`` reads: x_embedder / controlnet_x_embedder as Linears, separate q / k / v Linears (the k bias, which
    the engine drops, written as zeros), norm_q / norm_k / norm_added_q / norm_added_k, single blocks with proj_mlp and proj_out = [o_proj | fc2].
    Without single blocks the last text stream's post-attention half is written as zeros (to_add_out, ff_context, rows 2h .. 6h of
    norm1_context): the published file always holds it."""
    out = {}
    h, r = cfg.hidden_size, cfg.mlp_ratio
    dt = w["x_embedder.proj.weight"].dtype

    def put(name, t):
        out[name] = t.contiguous()

    for src, dst in (("x_embedder.proj", "x_embedder"), ("controlnet_x_embedder.proj", "controlnet_x_embedder")):
        put(dst + ".weight", w[src + ".weight"].reshape(h, -1))
        put(dst + ".bias", w[src + ".bias"])
    embedders = [("t_embedder", "timestep_embedder"), ("y_embedder", "text_embedder")] + ([("guidance_in", "guidance_embedder")] if cfg.guidance_embed else [])
    for leaf in ("weight", "bias"):
        shape = (lambda o, k: (o, k) if leaf == "weight" else (o,))
        put(f"context_embedder.{leaf}", w[f"context_embedder.{leaf}"])
        for src, dst in embedders:
            for n, m in ((0, 1), (2, 2)):
                put(f"time_text_embed.{dst}.linear_{m}.{leaf}", w[f"{src}.mlp.layers.{n}.{leaf}"])
        for i in range(cfg.depth_multimodal):
            pi, pt = (f"multimodal_transformer_blocks.{i}.{s}_transformer_block" for s in ("image", "text"))
            b = f"transformer_blocks.{i}"
            full = pt + ".attn.o_proj.weight" in w
            put(f"{b}.norm1.linear.{leaf}", w[f"{pi}.adaLN_modulation.layers.1.{leaf}"])
            ctx = w[f"{pt}.adaLN_modulation.layers.1.{leaf}"]
            if ctx.shape[0] == 2 * h:
                ctx = torch.cat([ctx, torch.zeros((4 * h,) + tuple(ctx.shape[1:]), dtype=dt)], dim=0)
            put(f"{b}.norm1_context.linear.{leaf}", ctx)
            for n, img_k, txt_k in (("q", "to_q", "add_q_proj"), ("k", "to_k", "add_k_proj"), ("v", "to_v", "add_v_proj")):
                for p, k in ((pi, img_k), (pt, txt_k)):
                    src = f"{p}.attn.{n}_proj.{leaf}"
                    put(f"{b}.attn.{k}.{leaf}", w[src] if src in w else torch.zeros(h, dtype=dt))
            put(f"{b}.attn.to_out.0.{leaf}", w[f"{pi}.attn.o_proj.{leaf}"])
            put(f"{b}.ff.net.0.proj.{leaf}", w[f"{pi}.mlp.fc1.{leaf}"])
            put(f"{b}.ff.net.2.{leaf}", w[f"{pi}.mlp.fc2.{leaf}"])
            put(f"{b}.attn.to_add_out.{leaf}", w[f"{pt}.attn.o_proj.{leaf}"] if full else torch.zeros(shape(h, h), dtype=dt))
            put(f"{b}.ff_context.net.0.proj.{leaf}", w[f"{pt}.mlp.fc1.{leaf}"] if full else torch.zeros(shape(r * h, h), dtype=dt))
            put(f"{b}.ff_context.net.2.{leaf}", w[f"{pt}.mlp.fc2.{leaf}"] if full else torch.zeros(shape(h, r * h), dtype=dt))
            put(f"controlnet_blocks.{i}.{leaf}", w[f"controlnet_blocks.{i}.{leaf}"])
            if leaf == "weight" and cfg.use_qk_norm:
                for p, qn, kn in ((pi, "norm_q", "norm_k"), (pt, "norm_added_q", "norm_added_k")):
                    put(f"{b}.attn.{qn}.weight", w[f"{p}.qk_norm.q_norm.weight"])
                    put(f"{b}.attn.{kn}.weight", w[f"{p}.qk_norm.k_norm.weight"])
        for i in range(cfg.depth_unified):
            p, b = f"unified_transformer_blocks.{i}.transformer_block", f"single_transformer_blocks.{i}"
            put(f"{b}.norm.linear.{leaf}", w[f"{p}.adaLN_modulation.layers.1.{leaf}"])
            for n in "qkv":
                src = f"{p}.attn.{n}_proj.{leaf}"
                put(f"{b}.attn.to_{n}.{leaf}", w[src] if src in w else torch.zeros(h, dtype=dt))
            put(f"{b}.proj_mlp.{leaf}", w[f"{p}.mlp.fc1.{leaf}"])
            if leaf == "weight":
                put(f"{b}.proj_out.weight", torch.cat([w[f"{p}.attn.o_proj.weight"], w[f"{p}.mlp.fc2.weight"]], dim=1))
                if cfg.use_qk_norm:
                    put(f"{b}.attn.norm_q.weight", w[f"{p}.qk_norm.q_norm.weight"])
                    put(f"{b}.attn.norm_k.weight", w[f"{p}.qk_norm.k_norm.weight"])
            else:
                put(f"{b}.proj_out.bias", w[f"{p}.attn.o_proj.bias"])
            put(f"controlnet_single_blocks.{i}.{leaf}", w[f"controlnet_single_blocks.{i}.{leaf}"])
    return out
