"""MMDiT-X (Stable Diffusion 3.5 medium) for the parity tests: the CPU oracle of the dual-attention block form and a writer of the
Stability checkpoint layout.

``MMDiTXOracle`` extends ``oracle.mmdit.OracleMMDiT`` -- the restatement pinned against the reference -- by the one block form the reference
lacks, from the published model definition (Stability's mmditx.py, diffusers' JointTransformerBlock(use_dual_attention=True)): blocks
``i < cfg.dual_attention_blocks`` chunk the image module's adaLN output nine ways and add a second attention over the image tokens alone.
Every other block, the embedders, the modulation cache and the final layer are the base class's.  Rounding points follow the base class:
one per Linear output, modulate, norm and gated add.  Arithmetic restatement only: no SD3.5-medium checkpoint has been run through it."""
import math

import torch

from oracle.mmdit import OracleMMDiT, affine_transform, rms_norm, sdpa


class MMDiTXOracle(OracleMMDiT):
    def _double_block(self, i, img, txt, tkey, rope):
        cfg, P = self.cfg, self.P
        if i >= cfg.dual_attention_blocks:
            return super()._double_block(i, img, txt, tkey, rope)
        assert cfg.depth_unified == 0 and rope is None, "MMDiT-X is an SD3-family model"
        pi = f"multimodal_transformer_blocks.{i}.image_transformer_block"
        pt = f"multimodal_transformer_blocks.{i}.text_transformer_block"
        skip_txt = i == cfg.depth_multimodal - 1
        ii = self._pre_sdpa(img, pi, tkey, 9)  # (chunks 0 .. 5: the row order of every block; 6 .. 8: shift / scale / gate of attn2)
        ti = self._pre_sdpa(txt, pt, tkey, 2 if skip_txt else 6)
        mod = ii["mod"]
        B, S_i, _ = img.shape
        H, D = cfg.num_heads, cfg.head_dim
        scale = 1.0 / math.sqrt(D)
        # attn2: the second modulation of the same LayerNorm, its own projections (k_proj WITH bias), its own QK-RMSNorm, image tokens only
        m2 = self.aq(affine_transform(img, mod[6], mod[7], cfg.layer_norm_eps, P), (pi, "qkv2"))
        q2, k2, v2 = (self._lin(m2, f"{pi}.attn2.{n}_proj").reshape(B, S_i, H, D).transpose(1, 2) for n in "qkv")
        if cfg.use_qk_norm:
            q2 = rms_norm(q2, self.w[pi + ".qk_norm2.q_norm.weight"], 1e-6, P)
            k2 = rms_norm(k2, self.w[pi + ".qk_norm2.k_norm.weight"], 1e-6, P)
        a2 = self._merge(sdpa(q2, k2, v2, scale, P))
        # the joint attention, SD3 order [image, text] (mmdit.py:607-625)
        q, k, v = (torch.cat([ii[n], ti[n]], dim=2) for n in "qkv")
        o = self._merge(sdpa(q, k, v, scale, P))
        o_img, o_txt = o[:, :S_i], o[:, S_i:]
        # image stream: x += gate_msa * o_proj(attn); x += gate_msa2 * attn2.o_proj(a2); then the MLP half of _post_sdpa
        x = P.r(img + P.r(self._lin(self.aq(o_img, (pi, "o")), pi + ".attn.o_proj") * mod[2]))
        x = P.r(x + P.r(self._lin(self.aq(a2, (pi, "o2")), pi + ".attn2.o_proj") * mod[8]))
        m = affine_transform(x, mod[3], mod[4], cfg.layer_norm_eps, P)
        h1 = self.gelu(self._lin(self.aq(m, (pi, "fc1")), pi + ".mlp.fc1"), P)
        img = P.r(x + P.r(mod[5] * self._lin(self.aq(h1, (pi, "fc2")), pi + ".mlp.fc2")))
        txt = None if skip_txt else self._post_sdpa(txt, o_txt, ti, pt, False)
        return img, txt


def to_stability_sd3(w, cfg, prefix="model.diffusion_model."):
    """Reference-named MMDiT weights (synth_mmdit_weights) -> the Stability checkpoint layout sd3_checkpoint_to_reference reads: fused qkv
    (the main attention's k bias, which the reference drops, written as zeros; attn2's k bias kept), OIHW patch conv, [1, T, h] pos_embed,
    the text stream of the last block pre-only."""
    out = {}
    h = cfg.hidden_size

    def put(name, t):
        out[prefix + name] = t.contiguous()

    put("pos_embed", w["x_pos_embedder.pos_embed.weight"][None])
    put("x_embedder.proj.weight", w["x_embedder.proj.weight"].permute(0, 3, 1, 2))
    put("x_embedder.proj.bias", w["x_embedder.proj.bias"])
    for leaf in ("weight", "bias"):
        put(f"context_embedder.{leaf}", w[f"context_embedder.{leaf}"])
        put(f"final_layer.linear.{leaf}", w[f"final_layer.linear.{leaf}"])
        put(f"final_layer.adaLN_modulation.1.{leaf}", w[f"final_layer.adaLN_modulation.layers.1.{leaf}"])
        for emb in ("t_embedder", "y_embedder"):
            for n in (0, 2):
                put(f"{emb}.mlp.{n}.{leaf}", w[f"{emb}.mlp.layers.{n}.{leaf}"])
    for i in range(cfg.depth_multimodal):
        for ck, ref in (("x_block", "image_transformer_block"), ("context_block", "text_transformer_block")):
            src, dst = f"multimodal_transformer_blocks.{i}.{ref}", f"joint_blocks.{i}.{ck}"
            put(dst + ".attn.qkv.weight", torch.cat([w[f"{src}.attn.{n}_proj.weight"] for n in "qkv"], dim=0))
            qb, vb = w[src + ".attn.q_proj.bias"], w[src + ".attn.v_proj.bias"]
            put(dst + ".attn.qkv.bias", torch.cat([qb, torch.zeros_like(qb), vb], dim=0))
            if cfg.use_qk_norm:
                put(dst + ".attn.ln_q.weight", w[src + ".qk_norm.q_norm.weight"])
                put(dst + ".attn.ln_k.weight", w[src + ".qk_norm.k_norm.weight"])
            for leaf in ("weight", "bias"):
                put(f"{dst}.adaLN_modulation.1.{leaf}", w[f"{src}.adaLN_modulation.layers.1.{leaf}"])
                if src + ".attn.o_proj.weight" in w:
                    put(f"{dst}.attn.proj.{leaf}", w[f"{src}.attn.o_proj.{leaf}"])
                    put(f"{dst}.mlp.fc1.{leaf}", w[f"{src}.mlp.fc1.{leaf}"])
                    put(f"{dst}.mlp.fc2.{leaf}", w[f"{src}.mlp.fc2.{leaf}"])
                if ck == "x_block" and i < cfg.dual_attention_blocks:
                    put(f"{dst}.attn2.qkv.{leaf}", torch.cat([w[f"{src}.attn2.{n}_proj.{leaf}"] for n in "qkv"], dim=0))
                    put(f"{dst}.attn2.proj.{leaf}", w[f"{src}.attn2.o_proj.{leaf}"])
            if ck == "x_block" and i < cfg.dual_attention_blocks and cfg.use_qk_norm:
                put(dst + ".attn2.ln_q.weight", w[src + ".qk_norm2.q_norm.weight"])
                put(dst + ".attn2.ln_k.weight", w[src + ".qk_norm2.k_norm.weight"])
    assert out[prefix + "joint_blocks.0.x_block.attn.qkv.weight"].shape == (3 * h, h)
    return out


def without_dual(w, cfg):
    """(config, weights) of the same model with the second attention taken out: dual_attention_blocks = 0, the first 6h adaLN rows of the dual
    image modules, no attn2 tensors"""
    from dataclasses import replace
    h = cfg.hidden_size
    out = {}
    for k, t in w.items():
        if ".attn2." in k or ".qk_norm2." in k:
            continue
        out[k] = t[:6 * h] if (".image_transformer_block.adaLN_modulation." in k and t.shape[0] == 9 * h) else t
    return replace(cfg, dual_attention_blocks=0), out
