"""Golden vectors for the HiSup training losses: the five lines of the reference's `EncoderDecoder.forward_train` (models/hisup/model_hisup.py:302-306)
called with the reference's own `sigmoid_l1_loss` (:27-37) in float64, weighted as its `LossReducer` (train/trainer_hisup.py:31-39) with the shipped
loss_weights, and torch.autograd's gradients of the weighted total with respect to the five maps.  B = 3, 19 x 23: image 1 has no junction pixel
(w == 0 -> 1), image 2 exactly one, image 0 no edges (zero afmap).  Build-container only (imports the reference); emits tests/golden/hisup_loss.npz
(arrays only)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_hisup_heads_golden import load_hisup  # noqa: E402
from tests import hisup_loss_ref as L  # noqa: E402

KEYS = ("loss_jloc", "loss_joff", "loss_mask", "loss_afm", "loss_remask")
WEIGHTS = {"loss_jloc": 8.0, "loss_joff": 0.25, "loss_mask": 1.0, "loss_afm": 0.1, "loss_remask": 1.0}      # config/model/hisup.yaml


def main():
    mh = load_hisup()
    B, H, W, seed = L.CASES["fixture"]
    inp = L.make_inputs(B, H, W, seed)
    jloc, joff, mask, afm, remask = [p.double().requires_grad_(True) for p in inp["pred"]]
    targets = {"jloc": inp["t_jloc"], "joff": inp["t_joff"].double(), "mask": inp["t_mask"], "afmap": inp["t_afm"].double()}
    loss_dict = {k: 0.0 for k in KEYS}
    loss_dict['loss_jloc'] += F.cross_entropy(jloc, targets['jloc'].squeeze(dim=1))
    loss_dict['loss_joff'] += mh.sigmoid_l1_loss(joff[:, :], targets['joff'], -0.5, targets['jloc'])
    loss_dict['loss_mask'] += F.cross_entropy(mask, targets['mask'].squeeze(dim=1).long())
    loss_dict['loss_afm'] += F.l1_loss(afm, targets['afmap'])
    loss_dict['loss_remask'] += F.cross_entropy(remask, targets['mask'].squeeze(dim=1).long())
    total = sum([WEIGHTS[k] * loss_dict[k] for k in WEIGHTS.keys()])
    total.backward()
    out = {"weights": np.array([WEIGHTS[k] for k in KEYS]), "losses": np.array([float(loss_dict[k].detach()) for k in KEYS]),
           "total": np.array(float(total.detach()))}
    for n, p, g in zip(L.NAMES, inp["pred"], (jloc, joff, mask, afm, remask)):
        out["pred." + n] = p.numpy()
        out["grad." + n] = g.grad.numpy()
    out.update({"t_jloc": inp["t_jloc"].numpy(), "t_joff": inp["t_joff"].numpy(), "t_mask": inp["t_mask"].numpy(), "t_afm": inp["t_afm"].numpy()})
    path = os.path.join(HERE, "hisup_loss.npz")
    np.savez_compressed(path, **out)
    print("losses", out["losses"], "total", float(out["total"]), "->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
