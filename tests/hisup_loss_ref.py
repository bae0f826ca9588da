"""Reference for the HiSup training losses and their gradients (models/hisup/model_hisup.py:302-306 weighted as train/trainer_hisup.py:31-39): the
reference's five lines under torch autograd in float64 (`val_losses` / `sigmoid_l1` of tests/hisup_predict_ref.py, which tests/test_hisup_predict_cpu.py
pins to the reference's own functions), the analytic restatement of the gradient formulas of include/p3hip.h in numpy, and the seeded input generator
the tests share.  tests/test_hisup_loss_cpu.py pins all three to tests/golden/hisup_loss.npz, the reference's own numbers.  Test infrastructure only."""
import functools

import numpy as np
import torch

from tests import hisup_predict_ref as R

NAMES = ("jloc", "joff", "mask", "afm", "remask")                # the maps in the order of the losses they enter (hisup.LOSS_KEYS)
CHANNELS = (3, 2, 2, 2, 2)
SCALES = (2.0, 1.0, 2.0, 1.0, 3.0)
WEIGHTS = (8.0, 0.25, 1.0, 0.1, 1.0)                             # config/model/hisup.yaml loss_weights in LOSS_KEYS order
SIGN_MARGIN = 1e-4


def make_inputs(B, H, W, seed):
    """-> dict(pred = [jloc, joff, mask, afm, remask] fp32 NCHW, t_jloc int64 [B,1,H,W], t_joff, t_mask, t_afm fp32).
    randn logits scaled by SCALES; 1 % junction pixels of classes 1 / 2; image 1 has no junction, image 2 exactly one, every other image at least one;
    t_afm[0] = 0 (an image without edges: afm - t_afm is the logit itself); mask density 0.3.
    Asserted: no junction-pixel residual |sigmoid(joff) - 0.5 - t_joff| (float64) is below SIGN_MARGIN, so an fp32 evaluation cannot flip a sign of
    the joff gradient.  (The afm sign needs no margin: an fp32 subtraction has the sign of the exact difference.)"""
    g = torch.Generator().manual_seed(seed)
    pred = [torch.randn(B, n, H, W, generator=g) * s for n, s in zip(CHANNELS, SCALES)]
    t_jloc = torch.zeros(B, 1, H, W, dtype=torch.long)
    hit = torch.rand(B, 1, H, W, generator=g) < 0.01
    t_jloc[hit] = torch.randint(1, 3, (int(hit.sum()),), generator=g)
    for b in range(B):
        if b == 1:
            t_jloc[b] = 0
        elif b == 2 or not t_jloc[b].any():
            t_jloc[b] = 0
            t_jloc[b].view(-1)[(H * W) // 2] = 1 + b % 2
    t_joff = (torch.rand(B, 2, H, W, generator=g) - 0.5) * (t_jloc > 0)
    t_mask = (torch.rand(B, 1, H, W, generator=g) < 0.3).float()
    t_afm = torch.randn(B, 2, H, W, generator=g)
    t_afm[0] = 0
    junction = (t_jloc > 0).expand(B, 2, H, W)
    if bool(junction.any()):
        margin = float((pred[1].double().sigmoid() - 0.5 - t_joff.double()).abs()[junction].min())
        assert margin >= SIGN_MARGIN, f"seed {seed}: a junction-pixel residual of {margin:.2e} lies below {SIGN_MARGIN}: choose another seed"
    return dict(pred=pred, t_jloc=t_jloc, t_joff=t_joff, t_mask=t_mask, t_afm=t_afm)


def targets_of(inp):
    return [inp["t_jloc"], inp["t_joff"], inp["t_mask"], inp["t_afm"]]


def reference(inp, weights=WEIGHTS, upstream=1.0, dtype=torch.float64):
    """the reference's five lines under autograd -> (losses [5], total, [d (upstream * total) / d map] * 5), all of `dtype`"""
    cast = (lambda t: t.double()) if dtype == torch.float64 else (lambda t: t)
    preds = [p.detach().to(dtype).requires_grad_(True) for p in inp["pred"]]
    if dtype == torch.float64:
        losses = R.val_losses(*preds, *targets_of(inp))
    else:                                                        # the same five lines without the float64 casts
        import torch.nn.functional as F
        tm = inp["t_mask"].squeeze(1).long()
        losses = torch.stack([F.cross_entropy(preds[0], inp["t_jloc"].squeeze(1)), R.sigmoid_l1(preds[1], cast(inp["t_joff"]), -0.5, inp["t_jloc"]),
                              F.cross_entropy(preds[2], tm), F.l1_loss(preds[3], cast(inp["t_afm"])), F.cross_entropy(preds[4], tm)])
    total = (losses * torch.tensor(weights, dtype=dtype)).sum()
    (total * upstream).backward()
    return losses.detach(), total.detach(), [p.grad for p in preds]


def joff_image_factor(t_jloc, exact):
    """H * W / c_b per image (0 where c_b = 0) as float64 [B,1,1,1].  exact=False evaluates it the way the reference does: sigmoid_l1_loss builds
    t / w from `t = (...).float()`, a FLOAT32 tensor, w = t.mean(3).mean(2), whatever the dtype of the logits, so its float64 results carry the fp32
    rounding of that one factor (about 1e-7 relative at 224 x 224)."""
    t = ((t_jloc == 1) | (t_jloc == 2))
    if exact:
        c_b = t.sum((1, 2, 3), keepdim=True).double()
        hw = t_jloc.shape[2] * t_jloc.shape[3]
        return torch.where(c_b > 0, hw / c_b.clamp_min(1), torch.zeros_like(c_b)).numpy()
    t = t.float()
    w = t.mean(3, True).mean(2, True)
    w[w == 0] = 1
    return (t / w).amax((1, 2, 3), keepdim=True).double().numpy()


def analytic_gradients(inp, weights=WEIGHTS, exact_factor=False):
    """numpy float64 restatement of the formulas p3hip.h gives for p3_hisup_train_loss -> [d total / d map] * 5.  exact_factor: see joff_image_factor;
    the kernel computes H * W / c_b from the integer count, i.e. the exact form."""
    p = [t.numpy().astype(np.float64) for t in inp["pred"]]
    tj = inp["t_jloc"].numpy()[:, 0]
    tm = inp["t_mask"].numpy()[:, 0].astype(np.int64)
    B, _, H, W = p[0].shape
    N = B * H * W

    def ce(logits, t, w):
        e = np.exp(logits - logits.max(1, keepdims=True))
        soft = e / e.sum(1, keepdims=True)
        onehot = np.stack([(t == c) for c in range(logits.shape[1])], 1).astype(np.float64)
        return w / N * (soft - onehot)

    s = 1.0 / (1.0 + np.exp(-p[1]))
    junction = ((tj == 1) | (tj == 2))[:, None].astype(np.float64)
    per_image = joff_image_factor(inp["t_jloc"], exact=exact_factor)
    d_joff = weights[1] / (2 * N) * per_image * junction * np.sign(s - 0.5 - inp["t_joff"].numpy().astype(np.float64)) * s * (1 - s)
    d_afm = weights[3] / (2 * N) * np.sign(p[3] - inp["t_afm"].numpy().astype(np.float64))
    return [ce(p[0], tj, weights[0]), d_joff, ce(p[2], tm, weights[2]), d_afm, ce(p[4], tm, weights[4])]


def grad_err(g, g64):
    """max|g - g64| / max|g64|; a map whose reference gradient is all zero must be all zero"""
    g, g64 = torch.as_tensor(g).double(), torch.as_tensor(g64).double()
    top = float(g64.abs().max())
    if top == 0.0:
        return 0.0 if not bool(g.any()) else float("inf")
    return float((g - g64).abs().max()) / top


# (B, H, W, seed) of the cases the GPU tests run; the seeds are draws for which make_inputs' margin assertion holds
CASES = {"odd": (3, 37, 41, 1), "one": (1, 1, 1, 1), "small": (4, 16, 16, 1), "full": (2, 224, 224, 1), "fixture": (3, 19, 23, 5)}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (inputs, (losses64, total64, grads64)) of CASES[name] with WEIGHTS, computed once per process; callers leave both unchanged"""
    B, H, W, seed = CASES[name]
    inp = make_inputs(B, H, W, seed)
    return inp, reference(inp)
