"""A dtype code that names no type is refused by every entry point that picks a template instantiation from it: P3_EUNSUP, "<entry>: dtype" in
p3_last_error_string(), and no launch - the refusal comes before any HIP call, so this runs without a GPU and the (host) buffers are never read."""
import ctypes

import pytest

P3_F32, P3_BF16, P3_EUNSUP = 0, 1, -4
BAD = 7


@pytest.fixture(scope="module")
def lib():
    from pixelspointspolygons_amd._lib import load
    from pixelspointspolygons_amd.build import build_library
    return load(build_library(verbose=False))


_BUF = ctypes.create_string_buffer(4096)          # every pointer argument: non-null host memory nobody dereferences
P = ctypes.addressof(_BUF)


class _Dropout(ctypes.Structure):                  # p3_dropout (include/p3hip.h)
    _fields_ = [("seed", ctypes.c_void_p), ("site", ctypes.c_uint), ("p", ctypes.c_float)]


_DROP = _Dropout(None, 0, 0.0)
PD = ctypes.addressof(_DROP)

# (entry, arguments with valid shapes and the bad code in place of one dtype); the stream is NULL
CASES = [
    ("p3_cast", (P, BAD, P, P3_F32, 8, None)),
    ("p3_cast", (P, P3_F32, P, BAD, 8, None)),
    ("p3_dropout_apply", (P, BAD, P, P3_F32, 8, 4, PD, None)),
    ("p3_dropout_apply", (P, P3_BF16, P, BAD, 8, 4, PD, None)),
    ("p3_pool_pos", (P, BAD, P, P, None, P3_F32, 1, 2, 8, 4, None)),
    ("p3_pool_pos", (P, P3_F32, P, P, None, BAD, 1, 2, 8, 4, None)),
    ("p3_pool_pos_bwd", (P, BAD, P, P3_F32, 1, 2, 8, 4, None)),
    ("p3_pool_pos_bwd", (P, P3_BF16, P, BAD, 1, 2, 8, 4, None)),
    ("p3_patchify", (P, P, 1, 3, 8, 8, 4, BAD, None)),
    ("p3_tokens_assemble", (P, 8, BAD, None, None, P, P, P, 1, 2, 8, None)),
    ("p3_embed_tokens", (P, P, P, P, None, 1, 2, 8, 0, BAD, None)),
    ("p3_embed_tokens_bwd", (P, BAD, P, P, None, 1, 2, 8, None)),
    ("p3_pair_mean", (P, P, 1, 5, 2, 8, BAD, None)),
    ("p3_pair_mean_bwd", (P, P, BAD, 1, 5, 2, 8, 0, None)),
    ("p3_add_pos", (P, P, P, 1, 2, 8, BAD, None)),
    ("p3_score_out", (P, BAD, P, P, P, P, P, 1, 2, 64, 0, None)),
    ("p3_nhwc_to_nchw", (P, 8, BAD, None, None, P, 1, 8, 4, None)),
    ("p3_pad_nhwc", (P, 8, BAD, None, None, 0, 8, 8, P, 1, 2, 2, None)),
    ("p3_affine_fix", (P, P, P, P, 2, 8, BAD, None)),
    ("p3_pair_stats_bwd", (P, P, P, P, P, P, 1, 2, 8, BAD, None)),
    ("p3_act_bwd", (P, BAD, P, P3_F32, P, P3_F32, 8, 1, 1.0, None)),
    ("p3_act_bwd", (P, P3_F32, P, BAD, P, P3_F32, 8, 1, 1.0, None)),
    ("p3_act_bwd", (P, P3_F32, P, P3_F32, P, BAD, 8, 1, 1.0, None)),
    ("p3_upsample_bilinear", (P, BAD, P, BAD, 1, 2, 2, 4, 4, 4, 4, 0, 4, None)),
    ("p3_upsample_bilinear", (P, P3_F32, P, P3_BF16, 1, 2, 2, 4, 4, 4, 4, 0, 4, None)),       # no kernel for unequal types
    ("p3_head1x1", (P, 256, BAD, P, P, P, P, 1, 0, 1.0, P, None, 0, 4, 4, None)),
    ("p3_nchw_to_nhwc", (P, P, 8, BAD, 1, 8, 4, None)),
    ("p3_patchify_ld", (P, P, 1, 3, 8, 8, 4, 64, BAD, None)),
    ("p3_ce_loss_bwd", (P, 8, P, 2, 8, -1, P, P, P, P, BAD, 8, 8, None)),
]


@pytest.mark.parametrize("entry,args", CASES, ids=[f"{e}-{i}" for i, (e, _) in enumerate(CASES)])
def test_a_code_that_names_no_type_is_refused_before_any_launch(lib, entry, args):
    lib.p3_cast(None, 0, None, 0, 1, None)          # leaves another entry's message behind
    rc = getattr(lib, entry)(*args)
    msg = lib.p3_last_error_string().decode()
    assert rc == P3_EUNSUP, (entry, rc, msg)
    assert entry in msg and "dtype" in msg, (entry, msg)


def test_fp32x3_is_no_storage_code_for_the_glue_entries(lib):
    """P3_F32X3 (2) is fp32 storage only where an entry says so (the pillar descriptor); the glue entries get storage codes and refuse it"""
    assert lib.p3_cast(P, 2, P, P3_F32, 8, None) == P3_EUNSUP
    assert lib.p3_affine_fix(P, P, P, P, 2, 8, 2, None) == P3_EUNSUP
