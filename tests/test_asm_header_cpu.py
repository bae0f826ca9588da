"""The inline-asm primitives hipcc cannot check (LDS-DMA, hand-counted s_waitcnt, the transposing LDS read) are written once, in csrc/gfx950_asm.h.
Outside it only the statements listed here may name them; a new kernel calls the header's functions instead of pasting the string."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pixelspointspolygons_amd", "csrc")
WORDS = ("global_load_lds", "ds_read_b64_tr", "s_waitcnt")
# file -> {word: count}.  s_waitcnt: the `s_waitcnt lgkmcnt(0)` statements whose "+v" operand list names that site's fragment registers
ALLOWED = {
    "gemm_tn.hip": {"s_waitcnt": 2}, "gemm_tn_dma.hip": {"s_waitcnt": 1}, "gemm_tn_x3.hip": {"s_waitcnt": 2},
    "mask2_dw_mma.hip": {"s_waitcnt": 1}, "mask2_dw_x3.hip": {"s_waitcnt": 1}, "pair_dw_mma.hip": {"s_waitcnt": 1},
    "gemm_x3_as.hip": {"global_load_lds": 1},       # the one-dword `touch` DMA (an L2 prefetch), used in that file only
    "decode_layer.hip": {"s_waitcnt": 1},           # __builtin_amdgcn_s_waitcnt(0): the full drain of the layer's generation reset, one place
}


def test_shared_inline_asm_lives_in_the_header_only():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) > 40 and os.path.join(CSRC, "gfx950_asm.h") in files
    found = {}
    for path in files:
        code = re.sub(r"//.*", "", open(path).read())
        counts = {w: code.count(w) for w in WORDS if w in code}
        if counts and os.path.basename(path) != "gfx950_asm.h":
            found[os.path.basename(path)] = counts
    assert found == ALLOWED
    for path in files:                               # and the "+v" waits are what the s_waitcnt entries are: no bare wait hides among them
        name, code = os.path.basename(path), re.sub(r"//.*", "", open(path).read())
        if name not in ("gfx950_asm.h", "decode_layer.hip"):
            assert len(re.findall(r'asm volatile\("s_waitcnt lgkmcnt\(0\)"\s*:\s*"\+v"', code)) == ALLOWED.get(name, {}).get("s_waitcnt", 0), name
