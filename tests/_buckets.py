"""The default aspect buckets as the tests see them: latent shapes, level shapes and token counts, derived from
`config.ImageConfig().supported_dims` and nothing else.

Not a test module (the leading underscore keeps it out of collection).  `supported_dims` entries are [width, height] in
pixels (1344 x 768 -> latent H x W = 96 x 168, the convention of the full-size tests' time ids); the list holds both
orientations of every bucket, so the SET of latent shapes does not depend on that reading.  The UNet has three levels:
the latent itself and two stride-2 down-samplings of it.  tests/test_host_buckets.py pins this table to the numbers the GPU
parametrizations hard-code, so a change to the bucket list cannot leave them behind."""
from __future__ import annotations

import importlib
from typing import Iterable, List, Tuple

CFG = importlib.import_module("sdxl-training-improvements_amd.config")

VAE_SCALE = 8
LEVELS = 3


def latent_shapes() -> List[Tuple[int, int]]:
    """(H, W) of every default bucket's latent, in the order of the config."""
    out = []
    for w_px, h_px in CFG.ImageConfig().supported_dims:
        assert w_px % VAE_SCALE == 0 and h_px % VAE_SCALE == 0, (w_px, h_px)
        out.append((h_px // VAE_SCALE, w_px // VAE_SCALE))
    return out


def level_shapes(H: int, W: int) -> List[Tuple[int, int]]:
    """[(H, W), (H/2, W/2), (H/4, W/4)]"""
    assert H % (1 << (LEVELS - 1)) == 0 and W % (1 << (LEVELS - 1)) == 0, (H, W)
    return [(H >> l, W >> l) for l in range(LEVELS)]


def level_tokens(H: int, W: int) -> Tuple[int, ...]:
    """pixels (= tokens of the transformer blocks) per sample at each level"""
    return tuple(h * w for h, w in level_shapes(H, W))


def all_level_shapes() -> List[Tuple[int, int]]:
    """every (H, W) any level of any bucket has"""
    return sorted({s for hw in latent_shapes() for s in level_shapes(*hw)})


def level_of(h: int, w: int) -> List[int]:
    """the levels at which some bucket has an h x w image ([] if none)"""
    return sorted({l for hw in latent_shapes() for l, s in enumerate(level_shapes(*hw)) if s == (h, w)})


def tokens_at_level(level: int) -> List[int]:
    return sorted({level_tokens(*hw)[level] for hw in latent_shapes()})


def non_transposed() -> List[Tuple[int, int]]:
    """one orientation per bucket pair (H <= W), the square bucket excluded"""
    return sorted({hw for hw in latent_shapes() if hw[0] < hw[1]})


def rows_multiples(tokens: Iterable[int], batches: Iterable[int] = (1, 2, 3, 4, 16)) -> List[int]:
    """row counts B * tokens a GEMM sees for the given batch sizes"""
    return sorted({b * t for t in tokens for b in batches})
