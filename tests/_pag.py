"""Perturbed-attention guidance for the parity tests: the masked attention reference, the CPU oracle of a model whose named blocks run their main
attention under the identity mask, the operator cases and the forward references.

The definition (include/dk_hip.h, dk_attention_identity_bf16): with F text tokens in front of the image tokens, a text query sees every key; an
image query sees the text keys and its own key, nothing else.  ``ref_identity_attention`` is ``tests/_footprint.ref_attention`` under that additive
mask.  ``PagOracle`` is ``tests/_mmditx.MMDiTXOracle`` whose main ``sdpa`` in the blocks of ``pag`` runs under it, in the oracle's own key order:
the oracle concatenates [image, text] for SD3 where the engine stores [text, image]; the mask is defined on token identity, so the result is the
same.  attn2 of a dual block is not perturbed (diffusers perturbs ``attn`` only).

``boost``: tests/_slg.boost's weights (every gate chunk of the named blocks x 8) make a SKIPPED block visible, but not a perturbed one: they amplify
the MLP's bf16 noise as much as the attention's signal, and with query-norm weights near 1 the synthetic attention is close to uniform, so the
masked and the full softmax average similar rows -- the perturbed fp32 oracle then sits 1.0 - 1.1 gates from the full one (0.029 against a gate of
0.029 on case b3, block 1).  Here the ATTENTION gate alone (chunk 2 of both streams) is scaled by 16 and the image stream's query-norm weight
by 8 (sharper image queries: what they attend to matters), powers of two, exact in every element type: 4.2 - 5.5 gates on every case and set, which
tests/test_pag_cpu.py asserts on the oracles alone before anything is compared with the GPU.  Arithmetic only, on synthetic weights: no checkpoint
has been run."""
import contextlib
import functools
import math

import torch

import oracle.mmdit as om
from diffusionkit_amd.weights import synth_mmdit_weights
from oracle.mmdit import Prec, embed_dtype
from tests import _mmditx, _slg
from tests._footprint import split_heads
from tests._mmditx import MMDiTXOracle
from tests._util import BF

F16 = torch.float16
NEG = float("-inf")

# (B, H, S_t, S_i), D = 64: the operator cases
OP_CASES = [(2, 3, 77, 256),   # F straddles a tile and block 0 is mixed
            (1, 2, 154, 35),   # block 0 is all text, block 1 is mixed and ragged
            (1, 4, 20, 96),    # one block; F < 64, so the straddling tile is also an own tile
            (2, 2, 128, 256),  # everything aligned; pure image blocks, text tiles deduplicated against nothing
            (1, 1, 1, 70),     # F = 1
            (1, 2, 64, 1),     # a single image row (it sees every key: the masked reference IS the plain one here)
            (1, 2, 77, 1024)]  # many image blocks, own tiles far from the text tiles
LOUD_CASES = [OP_CASES[0], OP_CASES[-1]]  # the image K rows x 4
D = 64


def identity_mask(S, F):
    """[S, S] additive: 0 where query s sees key t (s < F, or t < F, or t == s), -inf elsewhere"""
    s, t = torch.arange(S)[:, None], torch.arange(S)[None, :]
    return torch.where((s < F) | (t < F) | (s == t), 0.0, NEG)


def ref_identity_attention(qkv, H, D, F, scale=None, dtype=torch.float64):
    """attention over a packed [B, S, 3 H D] buffer, [text (F rows), image] order, under the identity mask -> [B, S, H D] in ``dtype``"""
    B, S, _ = qkv.shape
    q, k, v = split_heads(qkv.to(dtype), H, D)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    p = torch.softmax((q * scale) @ k.transpose(-1, -2) + identity_mask(S, F).to(dtype), dim=-1)
    return (p @ v).transpose(1, 2).reshape(B, S, H * D)


def op_inputs(case, dtype, loud=False, seed=30):
    """the packed qkv of an operator case, values representable in ``dtype``; ``loud``: the image K rows x 4"""
    B, H, S_t, S_i = case
    h = H * D
    qkv = torch.randn(B, S_t + S_i, 3 * h, generator=torch.Generator().manual_seed(seed))
    if loud:
        qkv[:, S_t:, h:2 * h] *= 4.0
    return qkv.to(dtype).float()


def spiked_inputs(dtype, B=1, H=2, S_t=77, S_i=200, seed=33):
    """(case, qkv): every image row's own key is its query x 8 (q_s . k_s dominates), so the running maximum jumps by far more than the
    rescale threshold in the own tile -- the last tile a pure image block visits"""
    h = H * D
    qkv = (torch.randn(B, S_t + S_i, 3 * h, generator=torch.Generator().manual_seed(seed)) * 0.5).to(dtype).float()
    qkv[:, S_t:, h:2 * h] = (qkv[:, S_t:, :h] * 8.0).to(dtype).float()
    return (B, H, S_t, S_i), qkv


# ---- the model oracle -----------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _masked_sdpa(S_i, S_t):
    """inside: the ``sdpa`` the block code of oracle.mmdit and tests/_mmditx calls runs under the identity mask when it is the joint attention (S_i +
    S_t tokens, [image, text] order); an attention over other token counts (attn2: the image tokens alone) is the plain one"""
    plain = om.sdpa
    s, t = torch.arange(S_i + S_t)[:, None], torch.arange(S_i + S_t)[None, :]
    mask = torch.where((s >= S_i) | (t >= S_i) | (s == t), 0.0, NEG)

    def sdpa(q, k, v, scale, P):
        if q.shape[2] != S_i + S_t:
            return plain(q, k, v, scale, P)
        sc = P.r(P.r(q * scale) @ k.transpose(-1, -2)) + mask
        return P.r(P.r(torch.softmax(sc, dim=-1)) @ v)

    om.sdpa = _mmditx.sdpa = sdpa
    try:
        yield
    finally:
        om.sdpa = _mmditx.sdpa = plain


class PagOracle(MMDiTXOracle):
    """``pag``: the double blocks whose main attention runs under the identity mask"""

    def __init__(self, cfg, w, P, pag=(), **kw):
        super().__init__(cfg, w, P, **kw)
        self.pag = frozenset(int(b) for b in pag)

    def _double_block(self, i, img, txt, tkey, rope):
        if i not in self.pag:
            return super()._double_block(i, img, txt, tkey, rope)
        assert self.cfg.depth_unified == 0 and rope is None and txt.shape[1] > 0, "perturbed attention is the SD3 family's"
        with _masked_sdpa(img.shape[1], txt.shape[1]):
            return super()._double_block(i, img, txt, tkey, rope)


G_GATE, G_QUERY = 16.0, 8.0


def boost(weights, cfg, blocks):
    """a copy of reference-named MMDiT ``weights`` with, in ``blocks``, the attention gate (rows [2h, 3h) of ``adaLN_modulation.layers.1``, weight
    and bias, both streams) x G_GATE and the image stream's ``qk_norm.q_norm.weight`` x G_QUERY"""
    out = dict(weights)
    h = cfg.hidden_size
    for i in blocks:
        for stream in ("image", "text"):
            for leaf in ("weight", "bias"):
                name = f"multimodal_transformer_blocks.{i}.{stream}_transformer_block.adaLN_modulation.layers.1.{leaf}"
                if 3 * h <= out[name].shape[0]:  # (the text stream of the last block has no gate)
                    t = out[name].clone()
                    t[2 * h:3 * h] *= G_GATE
                    out[name] = t
        name = f"multimodal_transformer_blocks.{i}.image_transformer_block.qk_norm.q_norm.weight"
        out[name] = out[name] * G_QUERY
    return out


def boosted_weights(cfg, pag, seed=1234):
    """the synthetic weights of ``cfg`` with the blocks of ``pag`` boosted, as drawn (bf16): what ``pack_mmdit`` takes"""
    return boost(synth_mmdit_weights(cfg, seed=seed), cfg, pag)


PAG_SETS = [(1,), (0,), (3,), (1, 2)]  # a dual block; a fork right behind the embedders; the last block, whose text stream stops early; two blocks
FORWARD = _slg.FORWARD
TS = _slg.TS


@functools.lru_cache(maxsize=None)
def forward_refs(case, pag, f16=False):
    """{"full": {...}, "pag": {...}}: tests/_slg.forward_refs with the perturbed model in the skip model's place, on the weights boosted on ``pag``"""
    cfg, n, Hl, Wl, S_t = FORWARD[case]
    named = boosted_weights(cfg, pag)
    wf = {k: (v.to(F16) if f16 else v).float() for k, v in named.items()}
    text, pooled, lat = _slg.forward_inputs(cfg, n, Hl, Wl, S_t)
    precs = {"fp32": (Prec(), dict(embed_prec=Prec(embed_dtype(cfg)))), "emu16": (Prec(F16), {}), "emubf": (Prec(BF), {})} if f16 else \
            {"fp32": (Prec(), {}), "emu": (Prec(BF), {})}
    res = {"full": {}, "pag": {}}
    for name, (P, kw) in precs.items():
        res["full"][name] = _slg._final(PagOracle(cfg, wf, P, (), **kw), pooled, lat, text)
        res["pag"][name] = _slg._final(PagOracle(cfg, wf, P, pag, **kw), pooled[:n], lat[:n], text[:n])
    return res


# ---- the pipeline cases: tests/_slg.py's, with the perturbed model as the third one ---------------------------------------------------------------
PIPE_CFG, PIPE_PAG = _slg.PIPE_CFG, (1, 2)
SCALE = 5.0  # (tests/_slg.py's 2.5 leaves the four-step loop 1.4 gates from the loop without the term; 5.0: see tests/test_pag_cpu.py)
PAG_KW = dict(pag_scale=SCALE, pag_layers=PIPE_PAG, pag_interval=_slg.WINDOW)


def pipe_oracles(P, f16=False, **kw):
    """(full model, perturbed model) on the boosted pipeline weights, sharing them"""
    wf = {k: (v.to(F16) if f16 else v).float() for k, v in boosted_weights(PIPE_CFG, PIPE_PAG).items()}
    return PagOracle(PIPE_CFG, wf, P, (), **kw), PagOracle(PIPE_CFG, wf, P, PIPE_PAG, **kw)
