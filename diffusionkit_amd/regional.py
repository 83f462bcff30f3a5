"""Regional prompts: the group words of ``ops.attention_groups`` from boxes and masks (host only, numpy).

One 32-bit word per token of the joint [text | image] sequence; query i sees key j iff their words share a bit.  With a base prompt and R <= 31
regions: bit 0 on the base prompt's text tokens and on every image token, bit r on region r's text tokens and on the image tokens inside region r.
Without a base prompt the text of region r carries bit r alone, and the image tokens share bit 0 among themselves unless ``isolate_image``.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

MAX_REGIONS = 31


def parse_region(spec: str, mask: bool = False) -> dict:
    """``--region "x0,y0,x1,y1:prompt"`` -> {"prompt", "box"}; ``--region-mask PATH:prompt`` (``mask``) -> {"prompt", "mask"}"""
    head, sep, prompt = spec.partition(":")
    if not sep or not prompt.strip():
        raise ValueError(f"region {spec!r}: expected {'PATH' if mask else 'x0,y0,x1,y1'}:prompt")
    if mask:
        return {"prompt": prompt, "mask": head}
    try:
        box = tuple(float(v) for v in head.split(","))
    except ValueError:
        box = ()
    if len(box) != 4 or not (box[0] < box[2] and box[1] < box[3]):
        raise ValueError(f"region {spec!r}: the box is x0,y0,x1,y1 in pixels with x0 < x1 and y0 < y1")
    return {"prompt": prompt, "box": box}


def region_cells(region: dict, gh: int, gw: int, cell: int = 16) -> np.ndarray:
    """bool [gh, gw]: the image tokens of a region.  A token belongs to a box if the centre of its ``cell``-pixel cell lies in it (x0 <= cx < x1,
    y0 <= cy < y1); to a mask (path, PIL image or array, any size) if the NEAREST-sampled pixel at that centre is non-zero."""
    cy, cx = (np.arange(gh) + 0.5) * cell, (np.arange(gw) + 0.5) * cell
    if region.get("box") is not None:
        x0, y0, x1, y1 = region["box"]
        return ((cy >= y0) & (cy < y1))[:, None] & ((cx >= x0) & (cx < x1))[None, :]
    m = region.get("mask")
    if m is None:
        raise ValueError("a region needs a box or a mask")
    if isinstance(m, str):
        from PIL import Image
        m = Image.open(m)
    m = np.asarray(m)
    if m.ndim == 3:
        m = m.max(axis=-1)
    ys = np.minimum((cy / (gh * cell) * m.shape[0]).astype(np.int64), m.shape[0] - 1)
    xs = np.minimum((cx / (gw * cell) * m.shape[1]).astype(np.int64), m.shape[1] - 1)
    return m[ys][:, xs] != 0


def region_words(regions: Sequence[dict], gh: int, gw: int, text_len: int, base: bool = True, isolate_image: bool = False,
                 cell: int = 16) -> np.ndarray:
    """uint32 [S], S = (base + len(regions)) * text_len + gh * gw: the words of one batch row, text first (the base prompt's tokens, if any, then each
    region's), then the row-major image tokens.  Raises a ValueError that names the rule: no region, more than 31, an image token in no region
    without a base prompt."""
    if not 1 <= len(regions) <= MAX_REGIONS:
        raise ValueError(f"regions: between 1 and {MAX_REGIONS} regions (one bit of the group word each, bit 0 is the base prompt's), got {len(regions)}")
    img = np.zeros((gh, gw), dtype=np.uint32)
    covered = np.zeros((gh, gw), dtype=bool)
    for r, region in enumerate(regions, start=1):
        cells = region_cells(region, gh, gw, cell)
        img[cells] |= np.uint32(1 << r)
        covered |= cells
    if not base and not covered.all():
        y, x = np.argwhere(~covered)[0]
        raise ValueError(f"regions: {int((~covered).sum())} image tokens lie in no region (first: row {y}, column {x}) and there is no base prompt "
                         "(region_base=False): they would attend to no text")
    if base or not isolate_image:
        img |= np.uint32(1)
    text = [np.full(text_len, 1 << r, dtype=np.uint32) for r in range(0 if base else 1, len(regions) + 1)]
    return np.concatenate(text + [img.reshape(-1)])
