"""SD3 ControlNet for the parity tests: the CPU oracles of the ControlNet (diffusers' SD3ControlNetModel layout) and of a main model that
takes its taps, and a writer of the diffusers checkpoint layout.

Both oracles extend ``oracle.mmdit.OracleMMDiT`` -- the restatement pinned against the reference -- by what the reference lacks, from the
published model definition (diffusers' SD3ControlNetModel.forward and SD3Transformer2DModel.forward):

  * ``ControlNetOracle``: the embedders, ``pos_embed_input`` on the control latent, every joint block, and ``controlnet_blocks.j`` on the image
    stream behind block j.  ``full_last=True`` runs the last block's text stream through its post-attention half as the published model does
    (it needs that half's tensors, ``with_full_last_block``); False stops the text stream after attention, as the engine does.  No tap reads
    the text stream behind the last block, so the taps are the same either way (tests/test_controlnet_cpu.py shows it).
  * ``ControlledOracle``: ``round_E(x + s * tap[floor(g n / depth)])`` on the image stream behind block g for g < depth - 1.

Rounding points follow the base class (one per Linear output, modulate, norm and gated add) and the engine's association of the two patch
embeddings: round(round(x_embedder(tokens)) + round(round(pos_embed_input(control tokens)) + pos)).  The published code rounds s * tap and the
sum separately; here the add is one rounding (include/dk_hip.h).  Arithmetic restatement only: no ControlNet checkpoint has been run."""
import torch

from oracle.mmdit import OracleMMDiT, linear


def tap_index(g: int, n_taps: int, depth: int) -> int:
    """the tap added behind block g: diffusers' int(g / (depth / n_taps)) in integers"""
    return g * n_taps // depth


class ControlNetOracle(OracleMMDiT):
    def __init__(self, cfg, weights, prec=None, full_last=False, **kw):
        super().__init__(cfg, weights, prec, **kw)
        self.full_last = full_last

    def _adaln_names(self):
        return [n for n in super()._adaln_names() if n != "final_layer"]

    def _tokens(self, x):
        cfg = self.cfg
        B, Hl, Wl, C = x.shape
        p = cfg.patch_size
        assert not cfg.patchify_via_reshape
        return x.reshape(B, Hl // p, p, Wl // p, p, C).permute(0, 1, 3, 2, 4, 5).reshape(B, (Hl // p) * (Wl // p), -1)

    def _pos(self, Hl, Wl):
        cfg = self.cfg
        p, mh = cfg.patch_size, cfg.max_latent_resolution
        h, w_ = Hl // p, Wl // p
        y0, x0 = (mh - h) // 2, (mh - w_) // 2
        pe = self.w["x_pos_embedder.pos_embed.weight"].reshape(mh, mh, -1)
        return pe[y0:y0 + h, x0:x0 + w_].reshape(1, h * w_, -1)

    def _double_block(self, i, img, txt, tkey, rope):
        cfg = self.cfg
        if not (self.full_last and i == cfg.depth_multimodal - 1):
            return super()._double_block(i, img, txt, tkey, rope)
        # the last block in full: the text stream's module has six rows and a post-attention half (SD3 order [image, text], mmdit.py:607-625)
        import math
        from oracle.mmdit import sdpa
        pi = f"multimodal_transformer_blocks.{i}.image_transformer_block"
        pt = f"multimodal_transformer_blocks.{i}.text_transformer_block"
        ii, ti = self._pre_sdpa(img, pi, tkey, 6), self._pre_sdpa(txt, pt, tkey, 6)
        S_i = img.shape[1]
        q, k, v = (torch.cat([ii[n], ti[n]], dim=2) for n in "qkv")
        o = self._merge(sdpa(q, k, v, 1.0 / math.sqrt(cfg.head_dim), self.P))
        return self._post_sdpa(img, o[:, :S_i], ii, pi, False), self._post_sdpa(txt, o[:, S_i:], ti, pt, False)

    def __call__(self, latent, text, timestep, control_latent, taps=None):
        """-> [N_c, B, S_i, h]; ``control_latent``: [B or 1, Hl, Wl, C].  ``taps``: optional dict that receives the streams (embed_img,
        embed_txt, double{i}_img, double{i}_txt) as OracleMMDiT's does."""
        cfg, P = self.cfg, self.P
        tkey = float(timestep)
        B, Hl, Wl, _ = latent.shape
        txt = self._lin(P.r(text), "context_embedder")
        wx, wc = self.w["x_embedder.proj.weight"], self.w["pos_embed_input.proj.weight"]
        ctrl = linear(self._tokens(P.r(control_latent)), wc.reshape(wc.shape[0], -1), self.w["pos_embed_input.proj.bias"], P)
        conde = P.r(ctrl + self._pos(Hl, Wl)).expand(B, -1, -1)
        img = P.r(linear(self._tokens(P.r(latent)), wx.reshape(wx.shape[0], -1), self.w["x_embedder.proj.bias"], P) + conde)
        if taps is not None:
            taps["embed_img"], taps["embed_txt"] = img.clone(), txt.clone()
        out = []
        for i in range(cfg.depth_multimodal):
            img, txt = self._double_block(i, img, txt, tkey, None)
            if taps is not None:
                taps[f"double{i}_img"] = img.clone()
                if txt is not None:
                    taps[f"double{i}_txt"] = txt.clone()
            out.append(self._lin(img, f"controlnet_blocks.{i}"))
        return torch.stack(out)


class ControlledOracle(OracleMMDiT):
    """``control`` = (taps [n, B, S_i, h], scale) or None; set it before a call"""
    control = None

    def _double_block(self, i, img, txt, tkey, rope):
        img, txt = super()._double_block(i, img, txt, tkey, rope)
        depth = self.cfg.depth_multimodal
        if self.control is not None and i < depth - 1:
            taps, s = self.control
            s = float(torch.tensor(s, dtype=torch.float32))  # (the engine's scalar is fp32)
            img = self.P.r(img + s * taps[tap_index(i, taps.shape[0], depth)])
        return img, txt


class ChainOracle:
    """ControlNetOracle -> taps -> ControlledOracle as ONE model for the oracle step loops (oracle.pipeline.cfg_denoise, tests' plan loops): every
    evaluation runs the ControlNet on the evaluation's own input, all CFG rows included, then the main model with its taps.  ``active``: one
    bool per model evaluation in call order (None: every evaluation is controlled); an inactive one is the plain main model."""

    def __init__(self, main, cn, control_latent, scale, active=None):
        self.main, self.cn, self.control_latent, self.scale = main, cn, control_latent, scale
        self.active, self.calls = active, 0

    def cache_modulation_params(self, pooled, timesteps):
        self.main.cache_modulation_params(pooled, timesteps)
        self.cn.cache_modulation_params(pooled, timesteps)

    def __call__(self, latent, text, timestep):
        on = True if self.active is None else self.active[self.calls]
        self.calls += 1
        self.main.control = (self.cn(latent, text, timestep, self.control_latent), self.scale) if on else None
        return self.main(latent, text, timestep)


def evaluations_active(plan, interval):
    """per row of a ``sampler.step_plan``: whether its evaluation is controlled -- the rows of one step share the step's decision"""
    from diffusionkit_amd.pipeline import controlnet_step_active
    n = sum(r.ends_step for r in plan)
    out, step = [], 0
    for r in plan:
        out.append(controlnet_step_active(step, n, interval))
        step += int(r.ends_step)
    return out


def with_full_last_block(w, cfg, seed=77):
    """``w`` (synth_mmdit_weights of a control-net config: the last text stream pre-only) plus the post-attention half of the last block's text
    stream as the published model has it: o_proj, the MLP, and a six-row adaLN Linear whose first 2h rows are the ones ``w`` holds"""
    h, r = cfg.hidden_size, cfg.mlp_ratio
    pt = f"multimodal_transformer_blocks.{cfg.depth_multimodal - 1}.text_transformer_block"
    g = torch.Generator().manual_seed(seed)
    dt = w[pt + ".attn.q_proj.weight"].dtype

    def rnd(*shape):
        return (torch.randn(*shape, generator=g) * 0.02).to(dt)

    out = dict(w)
    for name, o, i in ((".attn.o_proj", h, h), (".mlp.fc1", r * h, h), (".mlp.fc2", h, r * h)):
        out[pt + name + ".weight"], out[pt + name + ".bias"] = rnd(o, i), rnd(o)
    for leaf, tail in (("weight", (h,)), ("bias", ())):
        k = f"{pt}.adaLN_modulation.layers.1.{leaf}"
        assert w[k].shape[0] == 2 * h
        out[k] = torch.cat([w[k], rnd(4 * h, *tail)], dim=0)
    return out


def to_diffusers_sd3_controlnet(w, cfg):
    """Reference-named ControlNet weights (synth_mmdit_weights of a control-net config, or ``with_full_last_block`` of them) -> the diffusers
    SD3ControlNetModel layout ``sd3_controlnet_checkpoint_to_reference`` reads: separate q / k / v Linears (the k bias, which the engine drops,
    written as zeros), OIHW patch convs, [1, T, h] pos_embed.  Without the last text stream's post-attention half in ``w`` that half is written
    as zeros (to_add_out, ff_context, rows 2h .. 6h of norm1_context): the published file always holds it."""
    out = {}
    h, r = cfg.hidden_size, cfg.mlp_ratio

    def put(name, t):
        out[name] = t.contiguous()

    put("pos_embed.pos_embed", w["x_pos_embedder.pos_embed.weight"][None])
    for src, dst in (("x_embedder.proj", "pos_embed.proj"), ("pos_embed_input.proj", "pos_embed_input.proj")):
        put(dst + ".weight", w[src + ".weight"].permute(0, 3, 1, 2))
        put(dst + ".bias", w[src + ".bias"])
    for leaf in ("weight", "bias"):
        put(f"context_embedder.{leaf}", w[f"context_embedder.{leaf}"])
        for src, dst in (("t_embedder", "timestep_embedder"), ("y_embedder", "text_embedder")):
            for n, m in ((0, 1), (2, 2)):
                put(f"time_text_embed.{dst}.linear_{m}.{leaf}", w[f"{src}.mlp.layers.{n}.{leaf}"])
    for i in range(cfg.depth_multimodal):
        pi, pt = (f"multimodal_transformer_blocks.{i}.{s}_transformer_block" for s in ("image", "text"))
        b = f"transformer_blocks.{i}"
        full = pt + ".attn.o_proj.weight" in w
        dt = w[pi + ".attn.q_proj.weight"].dtype
        for leaf in ("weight", "bias"):
            shape = (lambda o, k: (o, k) if leaf == "weight" else (o,))
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
    return out
