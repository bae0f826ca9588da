"""FFL initial contours (csrc/contours.hip, p3_init_contours), the parts that need no GPU: the two sequential restatements of find_contours the GPU tests compare
with (tests/marching_ref.py) against the documentation example and against each other, and the C-ABI entry and wrappers' argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import marching_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p3hip.h")


def test_documentation_example_of_find_contours():
    """skimage's documentation: a = zeros((3, 3)); a[0, 0] = a[2, 2] = 1; find_contours(a, 0.5) -> [[0, .5], [.5, 0]] and [[2, 1.5], [1.5, 2]]"""
    a = np.zeros((3, 3))
    a[0, 0] = 1
    a[2, 2] = 1
    got = M.find_contours_ref(a, 0.5, positive_orientation="low")
    assert len(got) == 2
    assert np.array_equal(got[0], np.array([[0.0, 0.5], [0.5, 0.0]])) and np.array_equal(got[1], np.array([[2.0, 1.5], [1.5, 2.0]]))
    high = M.find_contours_ref(a, 0.5)          # what the reference asks for: every contour reversed
    assert np.array_equal(high[0], got[0][::-1]) and np.array_equal(high[1], got[1][::-1])


@pytest.mark.parametrize("name", sorted(M.cases()))
def test_the_two_references_agree(name):
    image, level = M.cases()[name]
    assert not M.has_level_pixels(image, level)
    joined, walked = M.find_contours_ref(image, level), M.link_by_edges_ref(image, level)
    assert M.same_contours(joined, walked)
    if min(image.shape) < 2:
        assert joined == []


def test_the_inputs_cover_what_they_are_meant_to():
    c = {k: M.find_contours_ref(*v) for k, v in M.cases().items()}
    closed = lambda cs: [bool(np.array_equal(x[0], x[-1])) for x in cs]
    assert len(c["serpentine96"]) == 1 and closed(c["serpentine96"]) == [True] and len(c["serpentine96"][0]) - 1 == 4324          # > 4096, 13 doubling rounds
    assert len(c["checkerboard12"]) == 72 and sum(closed(c["checkerboard12"])) == 50
    assert len(c["cross10x13"]) == 4 and not any(closed(c["cross10x13"]))
    for k in ("smooth33x20", "smooth64_l045"):
        assert any(closed(c[k])) and not all(closed(c[k])), k
    assert c["1x5"] == [] and c["5x1"] == [] and len(c["2x2"]) == 1 and len(c["2x9"]) > 1
    lv = M.level_valued()
    assert M.has_level_pixels(lv) and len(M.link_by_edges_ref(lv)) > 0


def test_entries_are_declared_exported_and_validate_before_any_device_work():
    from pixelspointspolygons_amd._lib import load
    from pixelspointspolygons_amd.build import build_library
    lib = load(build_library(verbose=False))
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    m = re.search(r"\bint\s+p3_init_contours\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
    assert m and len(m.group(1).split(",")) == 21
    assert re.search(r"\bint64_t\s+p3_init_contours_workspace_bytes\s*\(\s*int\s+B\s*,\s*int\s+H\s*,\s*int\s+W\s*\)\s*;", text)
    comment = [c for c in re.findall(r"/\*.*?\*/", raw, flags=re.S) if "FFL initial contours" in c]
    assert comment and "polygonize_utils.py:15-44" in comment[0]
    assert hasattr(lib, "p3_init_contours") and hasattr(lib, "p3_init_contours_workspace_bytes")
    n64, dbl = ctypes.c_int64, ctypes.c_double

    def call(B=1, H=8, W=8, nv=16, nc=8):
        return lib.p3_init_contours(None, n64(64), n64(8), n64(1), B, H, W, dbl(0.5), nv, nc, None, None, None, None, None, None, None, None, None, None, None)

    assert call() == -1 and b"p3_init_contours" in lib.p3_last_error_string()
    assert call(B=0) == -2 and call(H=0) == -2 and call(nv=-1) == -2 and call(B=4, H=1 << 14, W=1 << 14) == -2
    assert lib.p3_init_contours_workspace_bytes(1, 1, 5) == 0 and lib.p3_init_contours_workspace_bytes(1, 5, 1) == 0
    one, two = lib.p3_init_contours_workspace_bytes(1, 33, 20), lib.p3_init_contours_workspace_bytes(2, 33, 20)
    assert 0 < one < two <= 2 * one


def test_wrappers_refuse_host_tensors():
    from pixelspointspolygons_amd import hip, polygonize_acm as A
    x = torch.tensor(M.doc_example())[None]
    with pytest.raises(hip.P3Error):
        hip.init_contours(x)
    with pytest.raises(hip.P3Error):
        hip.init_contours_device(x)
    with pytest.raises(hip.P3Error):
        A.init_contours(x, 0.5)
    with pytest.raises(hip.P3Error):
        A.polygonize_device(torch.zeros(1, 1, 3, 3), torch.zeros(1, 4, 3, 3))
