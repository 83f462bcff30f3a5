"""Helpers of the regional-prompt tests (no GPU): group words from boxes, the float64 masked softmax, the operator layouts, the masked oracle."""
import numpy as np
import torch

from oracle import mmdit as om
from oracle.mmdit import OracleMMDiT


def groups_for(gh, gw, text_lens, boxes, base=True, cell=16, isolate_image=False):
    """uint32 [S] words of [text | image]: ``text_lens`` = token counts of (the base prompt, if ``base``, then) every region's prompt; an image token
    of the gh x gw grid lies in a box (x0, y0, x1, y1) iff its cell centre does (x0 <= cx < x1).  Bit 0: base text and image tokens; bit r: region r"""
    cy, cx = np.meshgrid((np.arange(gh) + 0.5) * cell, (np.arange(gw) + 0.5) * cell, indexing="ij")
    img = np.zeros((gh, gw), dtype=np.uint32)
    if base or not isolate_image:
        img |= np.uint32(1)
    for r, (x0, y0, x1, y1) in enumerate(boxes, start=1):
        img[(cx >= x0) & (cx < x1) & (cy >= y0) & (cy < y1)] |= np.uint32(1 << r)
    text = [np.full(n, 1 << (r if base else r + 1), dtype=np.uint32) for r, n in enumerate(text_lens)]
    return np.concatenate(text + [img.reshape(-1)])


def allowed(words):
    """bool [..., S, S] from uint32 words [..., S]"""
    w = np.asarray(words, dtype=np.uint32)
    return torch.from_numpy((w[..., :, None] & w[..., None, :]) != 0)


def masked_ref64(q, k, v, scale, mask):
    """float64 softmax over the allowed keys only (the others are removed before the softmax); q / k / v [G, S, D], mask bool [G, S, S]"""
    s = (q.double() @ k.double().transpose(1, 2) * scale).masked_fill(~mask, float("-inf"))
    return torch.softmax(s, dim=-1) @ v.double()


# S = 64 + 64 + 5.  Block 0 (rows 0..127) never visits tile 2 and block 1 (rows 128..132) visits tile 2 alone; rows 97..127 share their wave with row 96,
# which sees tile 0, and see nothing there themselves: their maximum is still unset when tile 0 is done; rows 64..95 are a whole wave that skips tile 0
_EMPTY_FIRST = np.array([1] * 64 + [2] * 32 + [3] + [2] * 31 + [4] * 5, dtype=np.uint32)[None]
# name -> (B, S, words [B, S]): the hazards of csrc/attention_group.hip (128-query blocks of four 32-query waves, 64-key tiles)
LAYOUTS = {
    "ragged_key_tile_and_query_block_S70": (1, 70, (1 + np.arange(70, dtype=np.uint32) % 3)[None]),
    "skipped_tiles_and_rows_with_empty_first_tile_S133": (1, 133, _EMPTY_FIRST),
    "all_full_S200": (1, 200, np.full((1, 200), 0xFFFFFFFF, dtype=np.uint32)),
    "words_differ_per_batch_row_S150": (2, 150, np.stack([1 + np.arange(150, dtype=np.uint32) // 50, 1 + np.arange(150, dtype=np.uint32) % 2 * 2])),
    "three_interleaved_groups_mostly_mixed_S300": (1, 300, (np.uint32(1) << (np.arange(300, dtype=np.uint32) % 3))[None]),
}


class RegionalOracle(OracleMMDiT):
    """the FLUX oracle whose joint attention, in every double and single block, is oracle.mmdit.sdpa with the scores the group words [B, S] disallow
    removed in front of the softmax (same rounding points)"""

    def __init__(self, cfg, weights, P, words):
        super().__init__(cfg, weights, P)
        self.mask = allowed(words)[:, None]

    def __call__(self, *args, **kw):
        plain, mask = om.sdpa, self.mask
        om.sdpa = lambda q, k, v, scale, P: P.r(P.r(torch.softmax(P.r(P.r(q * scale) @ k.transpose(-1, -2)).masked_fill(~mask, float("-inf")), dim=-1)) @ v)
        try:
            return super().__call__(*args, **kw)
        finally:
            om.sdpa = plain
