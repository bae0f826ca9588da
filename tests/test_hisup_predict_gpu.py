"""HiSup inference after the heads on the GPU: p3_hisup_junctions, p3_hisup_regions, p3_hisup_val_loss and the whole model's `forward_val`,
through the public wrappers.  References: tests/golden/hisup_predict.npz (the reference's own `get_pred_junctions` / loss functions),
tests/hisup_predict_ref.py (their restatement, pinned to the fixture by tests/test_hisup_predict_cpu.py) at 224 x 224, scipy.ndimage for the
regions.  Junction inputs are planted so that the comparison is exact and complete: no junction is excluded by a margin guard."""
import numpy as np
import pytest
import torch

from tests import guard as G
from tests import hisup_predict_ref as R
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _hip():
    from pixelspointspolygons_amd import hip
    return hip


def _run_junctions(jloc, joff, **kw):
    juncs, scores, index, counts = _hip().hisup_junctions(jloc.to(DEV), joff.to(DEV), **kw)
    return juncs.cpu(), scores.cpu(), index.cpu(), counts.cpu()


# ------------------------------------------------------------------------------------------------ 1. junctions: fixture and 224 x 224
def test_junctions_against_the_reference_fixture():
    d, _ = load_golden("hisup_predict.npz")
    ks = [int(k) for k in d["junc.k"]]
    jloc = torch.cat([torch.full_like(d["junc.jloc12"][:, :1], 6.0), d["junc.jloc12"]], 1)
    got = _run_junctions(jloc, d["junc.joff"])
    for i, K in enumerate(ks):
        ref = R.junctions(jloc[i], d["junc.joff"][i])
        R.check_planted(ref, K)
        assert torch.equal(ref["juncs"], d[f"junc.ref{i}"])
        k = min(K, 300)
        assert tuple(got[3][i].tolist()) == (k, k)
        assert torch.equal(got[2][i, :2 * k].long(), ref["index"])
        if k:
            assert float((got[0][i, :2 * k] - d[f"junc.ref{i}"]).abs().max()) <= 1e-4      # against the reference function's own output
            assert float((got[1][i, :2 * k].double() - ref["scores"]).abs().max()) <= 1e-6


# seeds: draws on which the three conditions of `check_planted` hold with this torch (about one seed in four does); they are re-checked below
@pytest.mark.parametrize("ks,seed", [((0,), 1), ((120,), 4), ((450,), 8), ((450, 0, 120, 33, 300), 7)])
def test_junctions_224_exact_and_complete(ks, seed):
    jloc, joff = R.planted_junction_maps(ks, 224, 4, 2, seed=seed)
    refs = [R.junctions(jloc[b], joff[b]) for b in range(len(ks))]
    for ref, K in zip(refs, ks):
        R.check_planted(ref, K)                                               # before anything is compared
    got = _run_junctions(jloc, joff)
    assert got[0].shape == (len(ks), 600, 2) and got[1].shape == (len(ks), 600) and got[3].shape == (len(ks), 2) and got[3].dtype == torch.int32
    for b, (ref, K) in enumerate(zip(refs, ks)):
        juncs, scores, index, counts = got
        k = min(K, 300)
        n = 2 * k
        assert tuple(counts[b].tolist()) == ref["counts"] == (k, k)
        assert torch.equal(index[b, :n].long(), ref["index"])                 # the same pixel at every rank; class-2 block first
        assert not juncs[b, n:].any() and not scores[b, n:].any() and bool((index[b, n:] == -1).all())
        if n:
            assert float((juncs[b, :n] - ref["juncs"]).abs().max()) <= 1e-4
            assert float((scores[b, :n].double() - ref["scores"]).abs().max()) <= 1e-6
            # the source pixel recovered from the coordinates alone: floor of the coordinate (offset + 0.5 lies in (0, 1))
            assert torch.equal(torch.floor(juncs[b, :n, 0]).long() + 224 * torch.floor(juncs[b, :n, 1]).long(), ref["index"])
            cls2 = jloc[b, 2].reshape(-1)[ref["index"][:k]]
            assert bool((cls2 >= 3).all())                                    # the first block really are the class-2 peaks


def test_junction_scales_multiply_the_coordinates():
    jloc, joff = R.planted_junction_maps((50,), 224, 4, 2, seed=4)
    a = _run_junctions(jloc, joff)
    b = _run_junctions(jloc, joff, scale_x=2.0, scale_y=0.5)
    assert torch.equal(a[2], b[2]) and torch.equal(a[0][..., 0] * 2.0, b[0][..., 0]) and torch.equal(a[0][..., 1] * 0.5, b[0][..., 1])


# ------------------------------------------------------------------------------------------------ 2. plateau and border, by hand
def test_junctions_plateau_border_and_suppressed_neighbour():
    H = W = 12
    jloc = torch.zeros(1, 3, H, W)
    jloc[0, 0] = 6.0
    jloc[0, 1:] = -2.0
    c2 = jloc[0, 2]
    # class 2: a two-pixel plateau, the four corners, one peak on each edge, and a peak (6, 6) whose neighbour (6, 7) is higher
    c2[3, 3] = c2[3, 4] = 5.0
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for i, (y, x) in enumerate(corners):
        c2[y, x] = 6.0 + i
    edges = [(0, 5), (5, 0), (H - 1, 6), (8, W - 1)]
    for i, (y, x) in enumerate(edges):
        c2[y, x] = 4.0 - 0.25 * i
    c2[6, 6], c2[6, 7] = 4.5, 4.75
    jloc[0, 1, 9, 3] = 5.5                                                    # class 1: one peak
    joff = torch.zeros(1, 2, H, W)                                            # sigmoid(0) - 0.5 = 0: coordinates are pixel + 0.5
    juncs, scores, index, counts = _run_junctions(jloc, joff)
    order2 = [(H - 1, W - 1), (H - 1, 0), (0, W - 1), (0, 0), (3, 3), (3, 4), (6, 7), (0, 5), (5, 0), (H - 1, 6), (8, W - 1)]
    assert counts[0].tolist() == [len(order2), 1]
    want = [y * W + x for y, x in order2] + [9 * W + 3]
    assert index[0, :len(want)].tolist() == want                              # plateau: both pixels, lower index first; (6, 6) suppressed
    assert 6 * W + 6 not in index[0].tolist()
    xy = torch.tensor([[x + 0.5, y + 0.5] for y, x in order2 + [(9, 3)]])
    assert torch.equal(juncs[0, :len(want)], xy)
    assert scores[0, 4] == scores[0, 5]


# ------------------------------------------------------------------------------------------------ 3. the cap
def test_junctions_cap_keeps_exactly_the_300_highest_per_class():
    jloc, joff = R.planted_junction_maps((450,), 224, 4, 2, seed=7)
    ref = R.junctions(jloc[0], joff[0])
    R.check_planted(ref, 450)
    juncs, scores, index, counts = _run_junctions(jloc, joff)
    assert counts[0].tolist() == [300, 300]
    p = jloc[0].double().softmax(0)
    for slot, c in enumerate((2, 1)):
        flat = p[c].reshape(-1)
        peaks = torch.nonzero(jloc[0, c].reshape(-1) >= 3).reshape(-1)
        assert len(peaks) == 450
        ranked = peaks[torch.argsort(flat[peaks], descending=True)]
        mine = index[0, slot * 300:(slot + 1) * 300].long()
        assert torch.equal(mine, ranked[:300])                                # rank 300 (index 299) is in ...
        assert int(ranked[300]) not in set(mine.tolist())                     # ... and rank 301 is out


# ------------------------------------------------------------------------------------------------ 4. layouts and repeatability
def test_junctions_both_layouts_and_two_runs_are_bit_identical():
    ks = (450, 7, 120)
    jloc, joff = R.planted_junction_maps(ks, 224, 4, 2, seed=16)
    B = len(ks)
    a = _run_junctions(jloc, joff)
    b = _run_junctions(jloc, joff)
    rows_l = torch.zeros(B * 224 * 224, 8)
    rows_o = torch.zeros(B * 224 * 224, 8)
    rows_l[:, :3] = jloc.permute(0, 2, 3, 1).reshape(-1, 3)
    rows_o[:, :2] = joff.permute(0, 2, 3, 1).reshape(-1, 2)
    rows_l[:, 3:] = 99.0                                                     # columns past the channels are not read
    c = _run_junctions(rows_l, rows_o, shape=(B, 224, 224))
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert a[3].tolist() == [[300, 300], [7, 7], [120, 120]]


def test_junction_wrapper_refuses_wrong_channels_and_oversized_maps():
    hip = _hip()
    with pytest.raises(hip.P3Error):
        hip.hisup_junctions(torch.zeros(1, 4, 8, 8, device=DEV), torch.zeros(1, 2, 8, 8, device=DEV))
    with pytest.raises(hip.P3Error):
        hip.hisup_junctions(torch.zeros(1, 3, 8, 8, device=DEV), torch.zeros(1, 2, 8, 9, device=DEV))
    with pytest.raises(hip.P3Error):
        hip.hisup_regions(torch.zeros(1, 3, 8, 8, device=DEV))
    big = torch.zeros(1, 2, 2048, 2049, device=DEV)
    with pytest.raises(hip.P3Error):
        hip.hisup_regions(big)


# ------------------------------------------------------------------------------------------------ 5. regions
def _planted_masks():
    n = 224
    m = {}
    a = np.zeros((n, n), bool)
    a[10:20, 10:20] = True; a[20:30, 20:30] = True                            # two blobs that touch only diagonally: one region
    a[40:80, 40:80] = True; a[50:70, 50:70] = False                           # a blob with a hole
    a[100, 100] = True                                                        # one pixel
    a[120:180, 20:30] = True; a[120:180, 60:70] = True; a[170:180, 20:70] = True      # U: the arms join only at the bottom
    a[0, 50:150] = True; a[n - 1, 30:90] = True; a[60:160, 0] = True; a[90:200, n - 1] = True   # along each border
    a[200:210, 100:110] = True; a[195:200, 110:120] = True                    # NE-diagonal contact
    m["shapes"] = a
    m["empty"] = np.zeros((n, n), bool)
    m["full"] = np.ones((n, n), bool)
    rs = np.random.RandomState(1)
    m["noise06"] = rs.rand(n, n) > 0.6
    return m


def _check_regions(out, b, logits, max_regions):
    mask64, labels, area, bbox, score = R.regions(logits)
    n = int(labels.max())
    assert int(out["n_regions"][b]) == n
    assert np.array_equal(out["labels"][b].cpu().numpy(), labels)             # exactly, numbering included
    k = min(n, max_regions)
    assert np.array_equal(out["area"][b, :k].cpu().numpy(), area[:k])
    assert np.array_equal(out["bbox"][b, :k].cpu().numpy(), bbox[:k])
    assert float(np.abs(out["mask"][b].cpu().numpy().astype(np.float64) - mask64).max()) <= 1e-6
    if k:
        rel = np.abs(out["score"][b, :k].cpu().numpy().astype(np.float64) - score[:k]) / score[:k]
        assert float(rel.max()) <= 1e-5, float(rel.max())
    assert not out["area"][b, k:].any()
    return n


def test_regions_planted_masks_against_scipy():
    hip = _hip()
    masks = _planted_masks()
    names = list(masks)
    logits = np.stack([R.planted_mask_logits(masks[k], seed=3 + i) for i, k in enumerate(names)])
    p = torch.from_numpy(logits).softmax(1)[:, 1]
    assert not bool(((p > 0.27) & (p < 0.73)).any())
    x = torch.from_numpy(logits).to(DEV)
    out = hip.hisup_regions(x)
    again = hip.hisup_regions(x)
    counts = {}
    for b, k in enumerate(names):
        counts[k] = _check_regions(out, b, logits[b], 1024)
    assert counts["empty"] == 0 and counts["full"] == 1 and counts["noise06"] == 844 and counts["shapes"] == 9
    assert int(out["area"][names.index("full"), 0]) == 224 * 224 and out["bbox"][names.index("full"), 0].tolist() == [0, 0, 224, 224]
    assert not out["status"].any()
    for k in ("mask", "labels", "n_regions", "area", "bbox", "score"):
        assert torch.equal(out[k], again[k]), k                               # bit for bit, the score included
    # token-major rows (stride 8) give the same as NCHW
    rows = torch.zeros(len(names) * 224 * 224, 8)
    rows[:, :2] = torch.from_numpy(logits).permute(0, 2, 3, 1).reshape(-1, 2)
    alt = hip.hisup_regions(rows.to(DEV), shape=(len(names), 224, 224))
    for k in ("mask", "labels", "n_regions", "area", "bbox", "score"):
        assert torch.equal(out[k], alt[k]), k


def test_regions_more_than_max_regions():
    hip = _hip()
    fg = np.random.RandomState(1).rand(224, 224) > 0.75
    logits = R.planted_mask_logits(fg, seed=9)[None]
    x = torch.from_numpy(logits).to(DEV)
    out = hip.hisup_regions(x, max_regions=4096)
    assert _check_regions(out, 0, logits[0], 4096) == 3094
    with pytest.raises(hip.P3Error, match="max_regions"):
        hip.hisup_regions(x)                                                  # the default 1024
    v, guards = G.guarded_set(dict(area=(1, 1024, torch.int32), bbox=(1024, 4, torch.int32), score=(1, 1024, torch.float32)), DEV)
    dev = hip.hisup_regions_device(x, max_regions=1024, out=v)          # the device-only path hands the status back; guard bands around the statistics
    assert dev["status"].tolist() == [1] and int(dev["n_regions"][0]) == 3094
    assert _check_regions(dev, 0, logits[0], 1024) == 3094                    # labels complete, statistics of the first 1024 regions
    for k, guard in guards.items():
        assert dev[k].data_ptr() == v[k].data_ptr()
        guard.check(written=True)
    two = hip.hisup_regions_device(torch.cat([x, -x.abs() * 0 + torch.tensor([3.0, -3.0], device=DEV).view(1, 2, 1, 1)]), max_regions=1024)
    assert two["status"].tolist() == [1, 0] and two["n_regions"].tolist() == [3094, 0]


# ------------------------------------------------------------------------------------------------ 6. validation losses
def test_val_losses_against_the_reference_fixture():
    hip = _hip()
    d, _ = load_golden("hisup_predict.npz")
    args = [d["loss.pred." + k] for k in ("jloc", "joff", "mask", "afm", "remask")] + [d["loss.t_jloc"], d["loss.t_joff"], d["loss.t_mask"], d["loss.t_afm"]]
    assert not d["loss.t_jloc"][1].any() and not d["loss.t_afm"][2].any()     # an image without junctions, an image without edges
    got = hip.hisup_val_loss(*[a.to(DEV) for a in args])
    again = hip.hisup_val_loss(*[a.to(DEV) for a in args])
    assert got.dtype == torch.float32 and got.shape == (5,) and torch.equal(got, again)
    rel = ((got.cpu().double() - d["loss.ref"]).abs() / d["loss.ref"].abs())
    print("val loss rel err", rel.tolist())
    assert float(rel.max()) <= 1e-5, rel.tolist()


def test_val_losses_224_batch_against_float64():
    hip = _hip()
    g = torch.Generator().manual_seed(3)
    B, S = 5, 224
    pred = [torch.randn(B, n, S, S, generator=g) * s for n, s in ((3, 2.0), (2, 1.0), (2, 2.0), (2, 1.0), (2, 3.0))]
    t_jloc = torch.zeros(B, 1, S, S, dtype=torch.long)
    hit = torch.rand(B, 1, S, S, generator=g) < 0.01
    t_jloc[hit] = torch.randint(1, 3, (int(hit.sum()),), generator=g)
    t_jloc[3] = 0
    t_joff = (torch.rand(B, 2, S, S, generator=g) - 0.5) * (t_jloc > 0)
    t_mask = (torch.rand(B, 1, S, S, generator=g) < 0.3).float()
    t_afm = torch.randn(B, 2, S, S, generator=g)
    t_afm[0] = 0
    ref = R.val_losses(*pred, t_jloc, t_joff, t_mask, t_afm)
    got = hip.hisup_val_loss(*[a.to(DEV) for a in pred + [t_jloc, t_joff, t_mask, t_afm]])
    rel = (got.cpu().double() - ref).abs() / ref.abs()
    assert float(rel.max()) <= 1e-5, rel.tolist()


# ------------------------------------------------------------------------------------------------ 7. the whole model
def _inputs(B, seed):
    from pixelspointspolygons_amd.synthetic import make_inputs
    d = make_inputs(B, seed=seed)
    lidar = torch.nested.nested_tensor_from_jagged(d["lidar_values"].to(DEV), d["lidar_offsets"].to(DEV))
    return d["image"].to(DEV), lidar


def _annotations(B, seed):
    g = torch.Generator().manual_seed(seed)
    anns = []
    for b in range(B):
        n = 0 if b == 1 else 12
        j = torch.rand(n, 2, generator=g) * 223.0
        edges = torch.stack([torch.arange(n), (torch.arange(n) + 1) % max(n, 1)], 1) if n else torch.zeros((0, 2), dtype=torch.long)
        mask = torch.zeros(224, 224)
        mask[30:90, 40:120] = 1
        anns.append(dict(junctions=j.to(DEV), juncs_tag=torch.randint(1, 3, (n,), generator=g).to(DEV), edges_positive=edges.to(DEV), mask=mask.to(DEV),
                         height=224, width=224, juncs_index=torch.zeros(n, dtype=torch.long), bbox=torch.tensor([[40.0, 30.0, 120.0, 90.0]])))
    return anns


@pytest.mark.parametrize("encoder,precision", [("vit_cnn", "fp32"), ("pointpillars_vit_cnn", "fp32"), ("early_fusion_vit_cnn", "fp32"), ("vit_cnn", "bf16")])
def test_whole_model_forward_val(encoder, precision):
    from pixelspointspolygons_amd import hip, hisup
    from pixelspointspolygons_amd.config import make_config
    torch.manual_seed(11)
    cfg = make_config(encoder, "hisup", vit_depth=1, precision=precision, device=DEV)
    model = hisup.HiSupModel(cfg, local_rank=0).eval()
    model.max_regions = 112 * 112                       # random weights: as many 8-connected regions as a 224 x 224 map can hold
    B = 2
    img, lidar = _inputs(B, seed=4)
    e = cfg.experiment.encoder
    x_img, x_lidar = (img if e.use_images else None), (lidar if e.use_lidar else None)
    # strict load of a reference-shaped state_dict (head keys from the fixture, see the CPU test for the encoder keys)
    head_keys = bytes(load_golden("hisup_predict.npz")[0]["keys.heads"].numpy()).decode().split("\n")
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert set(head_keys) == {k for k in sd if not k.startswith("encoder.")}
    model.load_state_dict({"encoder." + k[8:] if k.startswith("encoder.") else k: v for k, v in sd.items()}, strict=True)
    out_dev, loss0 = model.forward_val_device(x_img, x_lidar, None)
    assert loss0 == {k: 0.0 for k in hisup.LOSS_KEYS} and all(isinstance(v, float) for v in loss0.values())
    heads = out_dev["heads"]
    # the direct token-major hand-over against HiSupHeads fed the encoder's NCHW map
    feats = model.encoder(x_img, x_lidar) if (e.use_images and e.use_lidar) else model.encoder(x_img if e.use_images else x_lidar)
    assert feats.shape == (B, 256, 224, 224) and feats.dtype == torch.float32
    via_nchw = hisup.HiSupHeads.forward(model, feats)
    for k in ("joff", "jloc", "mask", "afm", "remask"):
        assert heads[k].shape == via_nchw[k].shape and heads[k].dtype == torch.float32
        if precision == "fp32":
            err = float((heads[k] - via_nchw[k]).abs().max() / via_nchw[k].abs().max())
            assert err <= 1e-6, (k, err)
    # the kernels called by hand on the returned maps (NCHW here, the model reads the predictors' token-major rows)
    juncs, scores, index, counts = hip.hisup_junctions(heads["jloc"], heads["joff"])
    reg = hip.hisup_regions_device(heads["remask"], model.max_regions)
    assert torch.equal(juncs, out_dev["juncs"]) and torch.equal(counts, out_dev["junc_counts"]) and torch.equal(index, out_dev["junc_index"])
    for k in ("labels", "n_regions", "area", "bbox", "score", "status"):
        assert torch.equal(reg[k], out_dev["regions"][k]), k
    assert torch.equal(reg["mask"], out_dev["mask"])
    # forward_val: documented keys, shapes and dtypes
    y = _annotations(B, seed=6)
    out, losses = model(x_img, x_lidar, y)
    assert set(out) == {"juncs_pred", "mask_pred", "regions"} and set(losses) == set(hisup.LOSS_KEYS)
    cnt = counts.cpu().numpy()
    for b in range(B):
        jp, mp, rg = out["juncs_pred"][b], out["mask_pred"][b], out["regions"][b]
        n = int(reg["n_regions"][b])
        assert isinstance(jp, np.ndarray) and jp.dtype == np.float32 and jp.shape == (int(cnt[b].sum()), 2)
        assert np.array_equal(jp, juncs[b, :jp.shape[0]].cpu().numpy())
        assert isinstance(mp, np.ndarray) and mp.dtype == np.float32 and mp.shape == (224, 224)
        assert set(rg) == {"labels", "area", "bbox", "score"}
        assert rg["labels"].shape == (224, 224) and rg["labels"].dtype == np.int32 and int(rg["labels"].max()) == n
        assert rg["area"].shape == (n,) and rg["bbox"].shape == (n, 4) and rg["score"].shape == (n,) and rg["score"].dtype == np.float32
        assert np.array_equal(rg["labels"], reg["labels"][b].cpu().numpy()) and int(rg["area"].sum()) == int((rg["labels"] > 0).sum())
    targets, _ = model.annotation_encoder(y)
    want = R.val_losses(*[heads[k].cpu() for k in ("jloc", "joff", "mask", "afm", "remask")], targets["jloc"].cpu(), targets["joff"].cpu(),
                        targets["mask"].cpu(), targets["afmap"].cpu())
    for i, k in enumerate(hisup.LOSS_KEYS):
        assert torch.is_tensor(losses[k]) and losses[k].is_cuda and losses[k].dim() == 0
        assert abs(float(losses[k]) - float(want[i])) <= 1e-5 * abs(float(want[i])), (k, float(losses[k]), float(want[i]))
    assert not targets["afmap"][1].any() and targets["afmap"][0].any()


def test_forward_val_refuses_other_mask_ratios_and_training():
    from pixelspointspolygons_amd import hisup
    from pixelspointspolygons_amd.config import make_config
    cfg = make_config("vit_cnn", "hisup", vit_depth=1, precision="bf16", device=DEV)
    model = hisup.HiSupModel(cfg, 0).eval()
    model.origin_height = model.origin_width = 448
    img, _ = _inputs(1, seed=2)
    with pytest.raises(NotImplementedError, match="cv2.resize"):
        model(img, None, None)
    with pytest.raises(NotImplementedError, match="training"):
        model.train()(img, None, None)
