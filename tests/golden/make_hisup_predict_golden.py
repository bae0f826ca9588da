"""Golden vectors for HiSup inference after the heads: the reference's own `get_pred_junctions` (models/hisup/polygon.py:26-38) called with
`forward_val`'s argument order (model_hisup.py:251-253,266), its `sigmoid_l1_loss` (:27-37) and the F.cross_entropy / F.l1_loss calls of
:241-245 in float64, and the state_dict keys of its `EncoderDecoder`.  Build-container only (imports the reference); emits
tests/golden/hisup_predict.npz (arrays only).  cv2 / skimage are stubs: nothing of them runs in these functions."""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_hisup_heads_golden import load_hisup, cfg, _Encoder  # noqa: E402
import hisup_predict_ref as R  # noqa: E402

JUNC_CASES = (0, 40, 330)          # K per image of the 96 x 96 junction fixture (stride-3 grid from pixel 1)


def main():
    mh = load_hisup()
    del sys.modules["pixelspointspolygons.models.hisup.polygon"]          # the real polygon.py (load_hisup left a stub for the head fixture)
    poly = importlib.import_module("pixelspointspolygons.models.hisup.polygon")
    out = {}
    # ---- junctions
    jloc, joff = R.planted_junction_maps(JUNC_CASES, 96, 3, 1, seed=11)
    out["junc.k"] = np.array(JUNC_CASES)
    out["junc.jloc12"] = jloc[:, 1:].numpy()          # class 0 is the constant 6.0
    out["junc.joff"] = joff.numpy()
    for i, K in enumerate(JUNC_CASES):
        R.check_planted(R.junctions(jloc[i], joff[i]), K)
        p = jloc[i].softmax(0)                          # jloc_pred.softmax(1) per image
        got = poly.get_pred_junctions(p[1:2], p[2:3], joff[i].sigmoid() - 0.5)     # (jloc_concave_pred[b], jloc_convex_pred[b], joff_pred[b])
        out[f"junc.ref{i}"] = np.asarray(got, dtype=np.float32).reshape(-1, 2)
        print("junctions K =", K, "->", out[f"junc.ref{i}"].shape)
    # ---- validation losses: B = 3; image 1 has no junction pixel (w == 0 branch), image 2 has no edges (zero afmap)
    g = torch.Generator().manual_seed(12)
    B, S = 3, 40
    pred = {"jloc": torch.randn(B, 3, S, S, generator=g) * 2, "joff": torch.randn(B, 2, S, S, generator=g), "mask": torch.randn(B, 2, S, S, generator=g) * 2,
            "afm": torch.randn(B, 2, S, S, generator=g), "remask": torch.randn(B, 2, S, S, generator=g) * 3}
    t_jloc = torch.zeros(B, 1, S, S, dtype=torch.long)
    hit = torch.rand(B, 1, S, S, generator=g) < 0.03
    t_jloc[hit] = torch.randint(1, 3, (int(hit.sum()),), generator=g)
    t_jloc[1] = 0
    t_joff = (torch.rand(B, 2, S, S, generator=g) - 0.5) * (t_jloc > 0)
    t_mask = (torch.rand(B, 1, S, S, generator=g) < 0.4).float()
    t_afm = torch.randn(B, 2, S, S, generator=g)
    t_afm[2] = 0
    d = lambda t: t.double()
    tm = t_mask.squeeze(dim=1).long()
    losses = [F.cross_entropy(d(pred["jloc"]), t_jloc.squeeze(dim=1)), mh.sigmoid_l1_loss(d(pred["joff"])[:, :], d(t_joff), -0.5, t_jloc),
              F.cross_entropy(d(pred["mask"]), tm), F.l1_loss(d(pred["afm"]), d(t_afm)), F.cross_entropy(d(pred["remask"]), tm)]
    for k, v in pred.items():
        out["loss.pred." + k] = v.numpy()
    out.update({"loss.t_jloc": t_jloc.numpy(), "loss.t_joff": t_joff.numpy(), "loss.t_mask": t_mask.numpy(), "loss.t_afm": t_afm.numpy(),
                "loss.ref": torch.stack(losses).numpy()})
    print("losses (jloc, joff, mask, afm, remask):", out["loss.ref"])
    # ---- state_dict keys of the reference's EncoderDecoder (over a parameter-free encoder: the head keys at the top level)
    c = cfg(256, 8)
    c["experiment"]["encoder"].update(in_height=8, in_width=8)
    keys = list(mh.EncoderDecoder(c, _Encoder()).state_dict().keys())
    out["keys.heads"] = np.frombuffer("\n".join(keys).encode(), dtype=np.uint8)          # newline-joined, as bytes (arrays only, no pickle)
    np.savez_compressed(os.path.join(HERE, "hisup_predict.npz"), **out)
    print("wrote hisup_predict.npz", os.path.getsize(os.path.join(HERE, "hisup_predict.npz")), "bytes,", len(keys), "head keys")


if __name__ == "__main__":
    main()
