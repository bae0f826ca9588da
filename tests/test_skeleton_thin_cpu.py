"""init_method "skeleton_device" (p3_skeleton_from_seg), the parts that need no GPU: the stated properties of the host restatement
(tests/skeleton_thin_ref.py) on the scenes of tests/skeleton_thin_cases.py, the figures a throwaway prototype of the definition gave for them, and the
argument checks of the C entry and its wrappers."""
import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from tests import skeleton_thin_cases as K
from tests import skeleton_thin_ref as R

EIGHT = np.ones((3, 3), dtype=bool)
TOPOLOGY_SCENES = tuple(n for n in K.SINGLE if n != "tiny") + ("scene224",)


def components_and_holes(img):
    """8-connected foreground components, 4-connected background components that do not reach the outside"""
    return ndi.label(img, structure=EIGHT)[1], ndi.label(~np.pad(img, 1))[1] - 1


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", TOPOLOGY_SCENES)
def test_the_skeleton_is_a_thin_subset_of_the_closed_mask_with_its_topology(name):
    for st in R.container_of(name).stages:
        assert not (st.thinned & ~st.closed).any()
        assert components_and_holes(st.thinned) == components_and_holes(st.closed)
        again, rounds = R.thin(st.thinned)
        assert np.array_equal(again, st.thinned) and rounds == 1


def test_tiny_blobs_shrink_to_nothing_or_to_a_pixel_without_a_link():
    """Zhang-Suen deletes a 2 x 2 block entirely (every pixel of it has B = 3, A = 1 and passes both sub-iterations' products), and the closed edge blob of the
    2 x 2 rectangle shrinks to such a block: the component count of the closed mask (2: the single pixel has no gradient above the level and gives no edge) is
    not kept here, so only subset and idempotence are asserted.  What remains, of the 3 x 3 rectangle, is one pixel without a link, which is no node."""
    c = R.container_of("tiny")
    st = c.stages[0]
    assert not (st.thinned & ~st.closed).any() and np.array_equal(R.thin(st.thinned)[0], st.thinned)
    assert components_and_holes(st.closed)[0] == 2 and components_and_holes(st.thinned)[0] == 1 and int(st.skeleton.sum()) == 1
    assert c.counts == (0, 0, 0, 0) and c.path_delim.tolist() == [0] and c.batch_delim.tolist() == [0, 0]


@pytest.mark.parametrize("name", K.SINGLE + K.EXTRA + ("batch3", "batch3_last", "scene224"))
def test_the_graph_and_the_paths_have_the_stated_properties(name):
    c = R.container_of(name)
    N, M, P, longest = c.counts
    assert c.pos.shape == (N, 2) and c.degrees.shape == (N,) and c.path_index.shape == (M,) and c.path_delim.shape == (P + 1,) and int(c.path_delim[-1]) == M
    idx, delim, deg = c.path_index.numpy(), c.path_delim.numpy(), c.degrees.numpy()
    n0, links = 0, []
    for st in c.stages:
        links += [(i + n0, j + n0) for i, j in st.links]
        n0 += len(st.nodes)
    assert n0 == N and len(set(links)) == len(links)
    assert np.array_equal(deg, np.bincount(np.array(links, dtype=np.int64).reshape(-1), minlength=N)) and (N == 0 or (1 <= deg.min() and deg.max() <= 4))
    on_paths, keys = [], []
    for p in range(P):
        path = idx[delim[p]:delim[p + 1]]
        assert len(path) >= 2 and (deg[path[1:-1]] == 2).all()
        assert (deg[path[0]] != 2 and deg[path[-1]] != 2) or (path[0] == path[-1] and path[0] == path.min() and path[1] < path[-2])
        on_paths += [(min(a, b), max(a, b)) for a, b in zip(path[:-1], path[1:])]
        keys.append((int(path[0]), int(path[1])))
    assert sorted(on_paths) == sorted(links)          # every link lies on exactly one path
    assert all(a < b for a, b in zip(keys[:-1], keys[1:]))
    assert M == len(links) + P and P <= len(links) <= 2 * N          # the capacities of the header comment
    assert np.array_equal(c.batch.numpy(), np.repeat(np.arange(len(c.stages)), [len(st.nodes) for st in c.stages]))
    assert c.batch_delim.tolist() == [0] + list(np.cumsum([len(st.paths) for st in c.stages]))


def test_the_scenes_give_the_figures_of_the_prototype():
    c = {n: R.container_of(n) for n in K.SINGLE}
    lens = lambda n: sorted(np.diff(c[n].path_delim.numpy()).tolist())
    hist = lambda n: np.bincount(c[n].degrees.numpy(), minlength=5).tolist()
    assert c["one"].counts == (52, 53, 1, 52) and hist("one") == [0, 0, 52, 0, 0]
    assert c["border"].counts[0] == 46 and lens("border") == [21, 25] and hist("border")[1] == 4
    assert c["touchcorner"].counts[0] == 75 and hist("touchcorner")[3:] == [0, 1] and lens("touchcorner") == [33, 45]
    assert c["theta"].counts[0] == 112 and hist("theta")[3:] == [2, 0] and lens("theta") == [14, 49, 53]
    assert c["thick"].stages[0].rounds == 5 and hist("thick")[3:] == [2, 0] and c["thick"].counts[2] == 3
    assert max(c[n].stages[0].rounds for n in K.SINGLE if n != "thick") <= 3          # only the bar needs more than three rounds
    assert c["tiny"].counts == (0, 0, 0, 0) and c["empty"].counts == (0, 0, 0, 0)
    assert c["noise"].counts[2] >= 8 and hist("noise")[1] >= 2 and hist("noise")[3] >= 2
    mid = R.container_of("batch3")
    assert mid.batch_delim.tolist() == [0, 1, 1, 3] and mid.counts[0] == 52 + 46
    last = R.container_of("batch3_last")
    assert last.batch_delim.tolist() == [0, 2, 2, 3] and last.counts == mid.counts and last.counts[3] == 52
    assert max(np.diff(R.container_of("border").path_delim.numpy())) == 25          # the longest path of the batch is not in its first image


def test_the_level_pixel_of_thick_is_not_above_the_level():
    seg = K.seg_of("thick")[0]
    assert float(seg[1][K.LEVEL_PIXEL]) == K.LEVEL and not R.edge_mask(seg, K.LEVEL)[K.LEVEL_PIXEL]
    above = seg.clone()
    above[1][K.LEVEL_PIXEL] = float(np.nextafter(np.float32(K.LEVEL), np.float32(1)))
    assert R.edge_mask(above, K.LEVEL)[K.LEVEL_PIXEL]
    assert R.container(above[None], K.LEVEL).counts != R.container_of("thick").counts          # a comparison that is not strict would show in the paths


@pytest.mark.parametrize("name", K.SINGLE + ("scene224",))
def test_the_edge_mask_equals_a_conv2d_formulation(name):
    seg = K.seg_of(name)[0]
    m = (K.LEVEL < seg[0]).float()[None, None]
    kx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]]) / 8
    grad = torch.nn.functional.conv2d(torch.nn.functional.pad(m, (1, 1, 1, 1), mode="replicate"), torch.stack([kx, kx.t()])[:, None])[0]
    g = (2 * grad).norm(dim=0)
    if seg.shape[0] >= 2:
        g = torch.clamp(seg[1] + g, 0, 1)
    assert np.array_equal(R.edge_mask(seg, K.LEVEL), (K.LEVEL < g).numpy())


# ---------------------------------------------------------------------------------------------------------------- the C entry, without a device
P3_EINVAL, P3_ESHAPE = -1, -2
# (B, H, W) -> bytes, recorded from the build that introduced the entry
WORKSPACE = [((0, 24, 29), 0), ((-2, 24, 29), 0), ((1, 1, 1), 1280), ((1, 24, 29), 2304), ((3, 30, 33), 7936), ((2, 64, 61), 16128), ((16, 224, 224), 1298944),
             ((1, 508, 508), 393472)]


def _lib():
    from pixelspointspolygons_amd._lib import lib
    return lib()


def test_the_header_declares_both_entries():
    from pixelspointspolygons_amd import _lib
    protos = _lib.prototypes()
    assert len(protos["p3_skeleton_from_seg"][1]) == 21 and len(protos["p3_skeleton_from_seg_workspace_bytes"][1]) == 3


def test_the_workspace_keeps_its_recorded_sizes():
    for args, nbytes in WORKSPACE:
        assert _lib().p3_skeleton_from_seg_workspace_bytes(*args) == nbytes, args


def test_skeleton_from_seg_refuses_bad_arguments_without_a_device():
    L = _lib()
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()
    args = lambda **kw: [kw.get(k, d) for k, d in (("seg", p), ("B", 1), ("C", 1), ("H", 24), ("W", 29), ("sb", 24 * 29), ("sc", 24 * 29), ("level", 0.5), ("max_nodes", 4),
                                                   ("max_slots", 5), ("max_paths", 1), ("out_pos", p), ("degrees", p), ("path_index", p), ("path_delim", p),
                                                   ("batch", p), ("batch_delim", p), ("counts", p), ("status", p), ("ws", p), ("stream", None))]
    for bad in (dict(H=509), dict(W=509), dict(C=0), dict(B=-1), dict(H=0), dict(W=0), dict(max_nodes=-1), dict(max_slots=-1), dict(max_paths=-1)):
        assert L.p3_skeleton_from_seg(*args(**bad)) == P3_ESHAPE, bad
        assert b"p3_skeleton_from_seg" in L.p3_last_error_string()
    for bad in ("seg", "out_pos", "degrees", "path_index", "path_delim", "batch", "batch_delim", "counts", "status", "ws"):
        assert L.p3_skeleton_from_seg(*args(**{bad: None})) == P3_EINVAL, bad


def test_the_wrappers_raise_on_host_tensors_and_bad_shapes():
    from pixelspointspolygons_amd import hip, polygonize_asm as A, polygonize_post as Q
    seg, cf = torch.zeros(1, 1, 8, 8), torch.zeros(1, 4, 8, 8)
    cfg = {**A.ASM_DEFAULTS, "init_method": "skeleton_device"}
    for call in (lambda: hip.skeleton_from_seg_device(seg), lambda: hip.skeleton_from_seg(seg, 0.5), lambda: A.init_skeletons(seg, method="skeleton_device"),
                 lambda: A.polygonize_device(seg, cf, cfg), lambda: Q.polygonize_asm_pieces(seg, cf, cfg), lambda: Q.polygonize_asm_polygons(seg, cf, cfg)):
        with pytest.raises(hip.P3Error):
            call()
    assert hip.skeleton_from_seg_capacity(2, 3, 5) == (30, 120, 60) and hip.SKELETON_THIN_MAX_SIDE + 4 == 512


def test_only_the_two_device_methods_are_taken():
    from pixelspointspolygons_amd import polygonize_asm as A
    seg, cf = torch.zeros(1, 1, 8, 8), torch.zeros(1, 4, 8, 8)
    assert A.ASM_DEFAULTS["init_method"] == "skeleton" and A.INIT_METHODS == ("marching_squares", "skeleton_device")
    with pytest.raises(NotImplementedError, match="skimage.*skan"):
        A.polygonize_device(seg, cf, A.ASM_DEFAULTS)
    with pytest.raises(NotImplementedError) as err:          # the earlier message word for word, then the pointer to the new method
        A.polygonize_device(seg, cf, A.ASM_DEFAULTS)
    assert str(err.value).startswith("init_method = 'skeleton': only \"marching_squares\" is built on the device; the skimage skeletonize / skan initialisation "
                                     "(\"skeleton\") is host code of the caller, whose skeletons optimize_skeletons takes") and "skeleton_device" in str(err.value)
    with pytest.raises(NotImplementedError, match="thinning"):
        A.polygonize_device(seg, cf, {**A.ASM_DEFAULTS, "init_method": "thinning"})
    with pytest.raises(ValueError, match="thinning"):
        A.init_skeletons(seg, method="thinning")
    with pytest.raises(ValueError):
        A.init_skeletons(seg, method="skeleton")
