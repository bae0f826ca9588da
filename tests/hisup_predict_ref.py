"""Restatement of what HiSup's `forward_val` does after the heads (models/hisup/model_hisup.py:241-293, models/hisup/polygon.py:8-38) in plain
torch on the CPU, for the tests of the HIP kernels, plus the generator of the planted inputs.  tests/test_hisup_predict_cpu.py pins
`junctions` and `val_losses` to the reference's own functions through tests/golden/hisup_predict.npz.  Test infrastructure only."""
import numpy as np
import torch
import torch.nn.functional as F

TH, TOPK = 0.008, 300


def planted_junction_maps(ks, size, stride, start, seed):
    """-> (jloc [B,3,size,size], joff [B,2,size,size]) fp32, one image per entry K of ks: class-0 logit 6, class-1 / class-2 logits 0.25 * randn,
    2K peaks on distinct cells of a grid (stride, first cell `start`), alternating between class 1 and class 2, heights a random permutation of
    linspace(3, 9, 2K); joff = randn."""
    g = torch.Generator().manual_seed(seed)
    n = len(range(start, size, stride))
    jl, jo = [], []
    for K in ks:
        jloc = torch.empty(3, size, size)
        jloc[0] = 6.0
        jloc[1:] = 0.25 * torch.randn(2, size, size, generator=g)
        if K:
            cells = torch.randperm(n * n, generator=g)[:2 * K]
            heights = torch.linspace(3, 9, 2 * K)[torch.randperm(2 * K, generator=g)]
            ys, xs = start + stride * (cells // n), start + stride * (cells % n)
            cls = 1 + (torch.arange(2 * K) % 2)
            jloc[cls, ys, xs] = heights
        jl.append(jloc)
        jo.append(torch.randn(2, size, size, generator=g))
    return torch.stack(jl), torch.stack(jo)


def _nms(a):
    ap = F.max_pool2d(a[None, None], 3, stride=1, padding=1)[0, 0]
    return a * (a == ap).float()


def junctions(jloc, joff):
    """one image: jloc [3,H,W], joff [2,H,W] fp32 logits -> dict(juncs fp32 [n,2], index int64 [n], scores float64 [n] (float64 softmax at the
    chosen pixels), counts (n_class2, n_class1), cand = per class the float32 probabilities of ALL candidates, sorted descending)."""
    H, W = jloc.shape[1:]
    p = jloc.float().softmax(0)
    p64 = jloc.double().softmax(0)
    off = joff.float().sigmoid() - 0.5
    juncs, index, scores, counts, cand = [], [], [], [], []
    for c in (2, 1):                                        # forward_val's argument order: class 2 first
        nms = _nms(p[c])
        flat = nms.reshape(-1)
        k = min(TOPK, int((nms > TH).sum()))
        s, idx = torch.topk(flat, k)
        y = (idx // W).float() + off[1].reshape(-1)[idx] + 0.5
        x = (idx % W).float() + off[0].reshape(-1)[idx] + 0.5
        juncs.append(torch.stack((x, y)).t().reshape(-1, 2))
        index.append(idx)
        scores.append(p64[c].reshape(-1)[idx])
        counts.append(k)
        cand.append(torch.sort(flat[flat > TH], descending=True).values)
    return dict(juncs=torch.cat(juncs), index=torch.cat(index), scores=torch.cat(scores), counts=tuple(counts), cand=cand,
                local_max=[_nms(p[c]).reshape(-1) for c in (2, 1)])


def check_planted(ref, K):
    """the three conditions under which the comparison is exact: K candidates per class, no local maximum within 8 % of the threshold, neighbouring
    sorted candidate scores at least 2.5e-4 apart (relative)"""
    for c in range(2):
        cand = ref["cand"][c].double()
        assert len(cand) == K, (len(cand), K)
        lm = ref["local_max"][c].double()
        lm = lm[lm > 0]
        assert bool(((lm / TH - 1).abs() > 0.08).all()), "a local maximum lies within 8 % of the threshold"
        if K > 1:
            gap = (cand[:-1] - cand[1:]) / cand[:-1]
            assert float(gap.min()) >= 2.5e-4, float(gap.min())


def sigmoid_l1(logits, targets, offset, mask):
    logp = torch.sigmoid(logits) + offset
    loss = torch.abs(logp - targets)
    t = ((mask == 1) | (mask == 2)).float()
    w = t.mean(3, True).mean(2, True)
    w[w == 0] = 1
    return (loss * (t / w)).mean()


def val_losses(jloc, joff, mask, afm, remask, t_jloc, t_joff, t_mask, t_afm):
    """float64 -> [loss_jloc, loss_joff, loss_mask, loss_afm, loss_remask] (model_hisup.py:241-245)"""
    d = lambda t: t.double()
    tm = t_mask.squeeze(1).long()
    return torch.stack([F.cross_entropy(d(jloc), t_jloc.squeeze(1)), sigmoid_l1(d(joff), d(t_joff), -0.5, t_jloc),
                        F.cross_entropy(d(mask), tm), F.l1_loss(d(afm), d(t_afm)), F.cross_entropy(d(remask), tm)])


def planted_mask_logits(fg, seed):
    """boolean foreground [H, W] -> remask logits [2, H, W]: logit difference +3 on the foreground, -3 elsewhere, 0.3 * randn noise on the
    difference, so that no probability lies in (0.27, 0.73)"""
    rs = np.random.RandomState(seed)
    d = np.where(fg, 3.0, -3.0) + 0.3 * np.clip(rs.randn(*fg.shape), -4, 4)
    base = rs.randn(*fg.shape)
    return np.stack([base - d / 2, base + d / 2]).astype(np.float32)


def regions(logits):
    """remask logits [2,H,W] -> (mask64, labels, area, bbox, score64) with scipy.ndimage (8-connected, raster-order numbering)"""
    from scipy import ndimage
    z = logits.astype(np.float64)
    e = np.exp(z - z.max(0))
    mask64 = e[1] / e.sum(0)
    l32 = torch.from_numpy(logits).softmax(0)[1].numpy()     # the fp32 decision the kernel makes
    labels, n = ndimage.label(l32 > 0.5, structure=np.ones((3, 3)))
    objs = ndimage.find_objects(labels)
    area = np.bincount(labels.ravel(), minlength=n + 1)[1:]
    bbox = np.array([[o[0].start, o[1].start, o[0].stop, o[1].stop] for o in objs], dtype=np.int64).reshape(-1, 4)
    score = np.asarray(ndimage.mean(mask64, labels, index=np.arange(1, n + 1)), dtype=np.float64).reshape(-1)
    return mask64, labels, area, bbox, score
