"""The scenes of the "skeleton_device" tests: filled rectangles (r0, c0, r1, c1) in channel 0 at value 1, level 0.5.  Small on purpose: W + 4 is 33 or 65, so
the pad straddles a word boundary of the bit-packed working image, and H != W.  seg_of(name) -> seg [B, C, H, W] fp32 on the host."""
import functools
import os
import sys

import numpy as np
import scipy.ndimage as ndi
import torch

LEVEL = 0.5

# name -> (H, W, C, rectangles)
RECTS = {
    "one": (24, 29, 1, [(5, 6, 17, 20)]),                                            # one cycle
    "border": (24, 29, 1, [(0, 0, 10, 12), (14, 15, 24, 29)]),                       # pad and crop; open paths that end on the image border
    "touchcorner": (30, 33, 1, [(4, 4, 12, 12), (12, 12, 22, 24)]),                  # a degree-4 node, two loops through it
    "theta": (24, 61, 2, [(4, 4, 18, 40)]),                                          # two degree-3 junctions, three paths
    "thick": (30, 33, 2, [(6, 6, 24, 27)]),                                          # a 9-pixel bar: 5 thinning rounds; a pixel exactly at the level
    "tiny": (24, 29, 1, [(5, 5, 6, 6), (10, 10, 12, 12), (15, 15, 18, 18)]),         # small blobs; one pixel without a link remains and is no node
    "empty": (24, 29, 1, []),
    # the sizes at which the kernels change: the smallest image (every Sobel tap clamps; channel 1 alone makes the edge), and the largest one (H + 4 = W + 4 =
    # 512: whole last words, two planes of exactly 64 KB, and no room for the link mask bytes in LDS: the walks read the bitmap itself)
    "sliver": (1, 5, 2, []),
    "max508": (508, 508, 2, [(3, 5, 200, 300), (300, 310, 508, 508), (250, 20, 260, 500), (200, 300, 240, 340)]),
    # the two sides of the threshold between the walks' two forms.  The workgroup asks for 8 (H+4) ceil((W+4)/32) + 64 bytes of LDS for the planes and, where
    # the sum stays within 160 KB - 512 = 163 328 bytes, (H+4)(W+4) more (rounded up to 4) for the link mask bytes.  At W = 350 (354 columns, 12 words a row) that
    # is 450 (H+4) + 64: 162 964 bytes at H = 358, the largest launch there is, and 163 414 at H = 359, the first image whose walks read the bitmap
    "links358": (358, 350, 2, [(2, 3, 150, 200), (180, 0, 358, 170), (200, 200, 340, 350), (100, 230, 170, 330)]),
    "bitmap359": (359, 350, 2, [(2, 3, 150, 200), (180, 0, 359, 170), (200, 200, 340, 350), (100, 230, 170, 330)]),
}
SINGLE = ("one", "border", "touchcorner", "theta", "thick", "tiny", "empty", "noise")
EXTRA = ("sliver", "max508", "links358", "bitmap359")
BATCH3 = ("one", "empty", "border")          # all 24 x 29, C = 1
BATCH3_LAST = ("border", "empty", "one")     # the longest path of the batch (the cycle of "one") lies in the last image, not in image 0
LEVEL_PIXEL = (8, 16)                        # of "thick", channel 1: exactly the level, so not above it; as an edge pixel it would bridge the outline and the bar


def _image(name):
    H, W, C, rects = RECTS[name]
    seg = np.zeros((C, H, W), dtype=np.float32)
    for r0, c0, r1, c1 in rects:
        seg[0, r0:r1, c0:c1] = 1.0
    if name == "theta":
        seg[1, 4:18, 21:24] = 0.9
    if name == "max508":
        seg[1, 100:103, 5:300] = 0.9          # a wall across the first rectangle: junctions for the walks that read the bitmap itself
    if name in ("links358", "bitmap359"):
        seg[1, 60:63, 3:200] = 0.9            # a wall across the first rectangle, and one that ends inside the second: junctions and a free end
        seg[1, 250:252, 0:90] = 0.9
    if name == "sliver":
        seg[1] = 1.0
    if name == "thick":
        seg[1, 10:19, 3:30] = 1.0
        seg[1][LEVEL_PIXEL] = LEVEL
    return seg


def _noise():
    """a seeded smooth field, 64 x 61: Gaussian-filtered normal noise thresholded at 0"""
    f = ndi.gaussian_filter(np.random.default_rng(11).normal(size=(64, 61)), 3.0)
    return (f > 0).astype(np.float32)[None]


def _bench_scene(B):
    """the first B images of the 224 x 224 scene of tools/bench_asm_init.py"""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    from bench_acm import synthetic
    return synthetic(B, seed=7)


@functools.lru_cache(maxsize=None)
def seg_of(name):
    if name == "batch3":
        return torch.cat([seg_of(n) for n in BATCH3])
    if name == "batch3_last":
        return torch.cat([seg_of(n) for n in BATCH3_LAST])
    if name == "noise":
        return torch.from_numpy(_noise())[None]
    if name == "scene224":
        return _bench_scene(1)[0].float().contiguous()
    return torch.from_numpy(_image(name))[None]


def frame_field(name, seed=23):
    """c0c2 [B, 4, H, W] for the chain tests: random directions and a small c2, as test_skeleton_init_gpu.py draws them"""
    B, _, H, W = seg_of(name).shape
    rng = np.random.default_rng(seed)
    theta = rng.uniform(0, np.pi, (B, H, W))
    c0, c2 = -np.exp(4j * theta), rng.normal(0, 0.05, (B, H, W)) + 1j * rng.normal(0, 0.05, (B, H, W))
    return torch.tensor(np.stack([c0.real, c0.imag, c2.real, c2.imag], 1), dtype=torch.float32)
