"""HiSup head set on the HIP path - mirror of the part of `EncoderDecoder` in
pixelspointspolygons/models/hisup/model_hisup.py:122-226 that follows the encoder: three 3-conv towers (`mask_head`, `jloc_head`,
`afm_head`), `joff_head` (MultitaskHead, one two-channel branch), two `ECA` gates, three predictors, `refuse_conv` and `final_conv`.
Same attribute / state_dict names, same forward_common outputs; the HRNet encoder and the polygonization stay out of scope.

Data flow on the device: the encoder's NCHW map becomes token-major [B*H*W, C] once; every 3x3 convolution is the implicit GEMM over a
zero-bordered image (p3_pad_nhwc + p3_gemm P3_A_CONV3X3 / conv_pad) with its BatchNorm statistics summed in the GEMM epilogue; a
BatchNorm + ReLU is never applied in a pass of its own: it travels as per-channel (scale, shift) to the kernel that reads the map next
(the next image builder, the ECA pool, the mixer).  Channel counts are padded to multiples of 32 with zero weights (the GEMM's K slice).
Forward only (eval and train-mode BatchNorm incl. the running-statistic updates); there is no hand-written backward for this head set.

The whole model for inference (second half of this file): `HiSupModel` (the reference's factory, model_hisup.py:312-360), `EncoderDecoder` (`HiSupHeads` + encoder;
`forward_val` of :229-293 on the device: csrc/hisup_predict.hip, and csrc/hisup_polygon.hip for the polygons) and `AnnotationEncoder` (:66-120).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import hip, ops
from .ffl import EarlyFusionViTCNN, PointPillarsViTCNN, ViTCNN, _khwc
from .vision_transformer import compute_dtype, is_split


def _up32(c):
    return (c + 31) // 32 * 32


class ECA(nn.Module):
    """model_hisup.py:38-64 (parameter container; `HiSupHeads._eca` runs it)"""

    def __init__(self, channel, gamma=2, b=1):
        super().__init__()
        t = int(abs((math.log(channel, 2) + b) / gamma))
        k = t if t % 2 else t + 1
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.conv = nn.Conv1d(1, 1, kernel_size=k, padding=int(k / 2), bias=False)
        self.sigmoid = nn.Sigmoid()
        self.out_conv = nn.Sequential(nn.Conv2d(channel, channel, kernel_size=1, padding=0, bias=False), nn.BatchNorm2d(channel), nn.ReLU(inplace=True))


class MultitaskHead(nn.Module):
    """models/hisup/multi_task_head.py: one Conv3x3 -> ReLU -> Conv1x1 branch per entry of head_size (the model uses [[2]])"""

    def __init__(self, input_channels, num_class, head_size):
        super().__init__()
        m = int(input_channels / 4)
        heads = []
        for output_channels in sum(head_size, []):
            heads.append(nn.Sequential(nn.Conv2d(input_channels, m, kernel_size=3, padding=1), nn.ReLU(inplace=True),
                                       nn.Conv2d(m, output_channels, kernel_size=1)))
        self.heads = nn.ModuleList(heads)
        assert num_class == sum(sum(head_size, []))


class HiSupHeads(nn.Module):
    """`EncoderDecoder` of model_hisup.py without encoder / annotation encoder / losses: __init__ builds the same submodules under the
    same names (load_state_dict of the reference's head weights is strict-compatible), `forward(features)` = lines 205-226."""

    def __init__(self, cfg=None, dim_in=None, precision=None):
        super().__init__()
        if dim_in is None:
            dim_in = int(cfg.experiment.model.decoder.in_feature_dim)
        self.dim_in = dim_in
        self.cd = compute_dtype(cfg) if precision is None and cfg is not None else (torch.float32 if precision in ("fp32", "float32", "fp32x3") else torch.bfloat16)
        hip.scope_module(self, is_split(cfg) if precision is None and cfg is not None else precision == "fp32x3")
        self.mask_head = self._make_conv(dim_in, dim_in, dim_in)
        self.jloc_head = self._make_conv(dim_in, dim_in, dim_in)
        self.afm_head = self._make_conv(dim_in, dim_in, dim_in)
        self.joff_head = MultitaskHead(dim_in, 2, head_size=[[2]])
        self.a2m_att = ECA(dim_in)
        self.a2j_att = ECA(dim_in)
        self.mask_predictor = self._make_predictor(dim_in, 2)
        self.jloc_predictor = self._make_predictor(dim_in, 3)
        self.afm_predictor = self._make_predictor(dim_in, 2)
        self.refuse_conv = self._make_conv(2, dim_in // 2, dim_in)
        self.final_conv = self._make_conv(dim_in * 2, dim_in, 2)

    @staticmethod
    def _make_conv(dim_in, dim_hid, dim_out):
        return nn.Sequential(nn.Conv2d(dim_in, dim_hid, kernel_size=3, padding=1), nn.BatchNorm2d(dim_hid), nn.ReLU(inplace=True),
                             nn.Conv2d(dim_hid, dim_hid, kernel_size=3, padding=1), nn.BatchNorm2d(dim_hid), nn.ReLU(inplace=True),
                             nn.Conv2d(dim_hid, dim_out, kernel_size=3, padding=1), nn.BatchNorm2d(dim_out), nn.ReLU(inplace=True))

    @staticmethod
    def _make_predictor(dim_in, dim_out):
        m = int(dim_in / 4)
        return nn.Sequential(nn.Conv2d(dim_in, m, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(m, dim_out, kernel_size=1))

    # ------------------------------------------------------------------------------------------ building blocks
    def _image(self, x, c, aff=None):
        """token-major map [R, ld] (first c channels valid) -> zero-bordered image [B, H+2, W+2, up32(c)], BatchNorm + ReLU applied when aff"""
        B, H, W = self._bhw
        sc, sh = aff if aff is not None else (None, None)
        return hip.pad_nhwc(x, x.stride(0), sc, sh, c if aff is not None else 0, c, _up32(c), B, H, W)

    def _conv3(self, xpad, cin, conv, act=hip.ACT_NONE, stats=False):
        """3x3 / pad 1 convolution of a zero-bordered image -> ([R, up32(Co)] with Co valid columns (the rest zero), sums or None)"""
        B, H, W = self._bhw
        co, cp = conv.out_channels, _up32(conv.out_channels)
        w2 = ops.shadow(conv.weight, self.cd, key="khwc32", fn=lambda t: _khwc(t, _up32(cin)))
        out = torch.zeros((B * H * W, cp), dtype=self.cd, device=xpad.device)
        sums = torch.zeros(2 * co, dtype=torch.float32, device=xpad.device) if stats else None
        hip.gemm(xpad, w2, bias=conv.bias.detach() if conv.bias is not None else None, act=act, a_mode=hip.A_CONV3X3, conv=(B, H, W, _up32(cin)),
                 lda=_up32(cin), conv_pad=True, M=B * H * W, out=out[:, :co], colsum=sums[:co] if stats else None, colsumsq=sums[co:] if stats else None)
        return out, sums

    def _bn(self, sums, bn):
        B, H, W = self._bhw
        training = self.training
        r = hip.bn_finalize(sums, float(B * H * W) * (ops.sync_stats(sums) if training else 1), bn.weight.detach(), bn.bias.detach(), bn.running_mean,
                            bn.running_var, bn.eps, bn.momentum, training)
        if training:
            ops.bump_batches_tracked(bn)
        return r

    def _tower(self, xpad, cin, seq):
        """`_make_conv` stack (model_hisup.py:149-161): returns the LAST conv's raw output + its pending (scale, shift)"""
        a, aff = None, None
        for ci, bi in ((0, 1), (3, 4), (6, 7)):
            if a is not None:
                xpad, cin = self._image(a, seq[ci].in_channels, aff), seq[ci].in_channels
            a, sums = self._conv3(xpad, cin, seq[ci], stats=self.training)
            aff = self._bn(sums, seq[bi])
        return a, aff

    def _predictor(self, xpad, cin, seq):
        """`_make_predictor` / MultitaskHead branch: Conv3x3 -> ReLU -> Conv1x1 -> fp32 [R, n_out] (row stride 8)"""
        h, _ = self._conv3(xpad, cin, seq[0], act=hip.ACT_RELU)
        n = seq[2].out_channels
        w = ops.shadow(seq[2].weight, self.cd, key="1x1p32", fn=lambda t: ops._pad_cols(t.reshape(t.shape[0], -1), _up32(t.shape[1])))
        out = torch.zeros((h.shape[0], 8), dtype=torch.float32, device=h.device)
        hip.gemm(h, w, bias=seq[2].bias.detach(), out=out[:, :n])
        return out, n

    def _eca(self, a1, aff1, a2, aff2, mod):
        """ECA.forward(x1, x2) with x = relu(bn(a)) pending: gate from the pooled sum, x2 * gate -> Conv1x1 (no bias) -> BatchNorm (+ ReLU pending)"""
        B, H, W = self._bhw
        C = self.dim_in
        gate = hip.eca_gate(a1, aff1, a2, aff2, mod.conv.weight, B, H * W, C)
        xg = torch.zeros((a2.shape[0], _up32(C)), dtype=self.cd, device=a2.device)
        hip.affine_relu_mix(xg, a2, aff2, H * W, C, gate=gate)
        conv, bn = mod.out_conv[0], mod.out_conv[1]
        w = ops.shadow(conv.weight, self.cd, key="1x1p32", fn=lambda t: ops._pad_cols(t.reshape(t.shape[0], -1), _up32(t.shape[1])))
        z = torch.zeros((a2.shape[0], _up32(C)), dtype=self.cd, device=a2.device)
        sums = torch.zeros(2 * C, dtype=torch.float32, device=a2.device) if self.training else None
        hip.gemm(xg, w, out=z[:, :C], colsum=sums[:C] if self.training else None, colsumsq=sums[C:] if self.training else None)
        return z, self._bn(sums, bn)

    def _nchw(self, x, n, aff=None):
        B, H, W = self._bhw
        sc, sh = aff if aff is not None else (None, None)
        return hip.nhwc_to_nchw(x, x.stride(0), sc, sh, B, n, H * W).view(B, n, H, W)

    # ------------------------------------------------------------------------------------------ forward_common after the encoder
    @torch.no_grad()
    def forward(self, features):
        """features: the encoder's NCHW fp32 map [B, dim_in, H, W] -> dict(joff, jloc, mask, afm, remask) NCHW fp32, the tensors
        `forward_common` returns (model_hisup.py:207-226)."""
        hip._dev(features)
        B, C, H, W = features.shape
        if C != self.dim_in:
            raise hip.P3Error(f"HiSupHeads: expected {self.dim_in} feature channels, got {C}")
        return self._heads(hip.nchw_to_nhwc(features, self.cd, _up32(C)), None, B, H, W)

    @torch.no_grad()
    def _heads(self, F_, F_aff, B, H, W):
        """the head set on a token-major feature map [B*H*W, >= dim_in] in the compute dtype; F_aff = (scale, shift) of a BatchNorm + ReLU that is
        still pending on it (the `*_vit_cnn` encoders' `features_nhwc`), None for a finished map."""
        C = self.dim_in
        self._bhw = (B, H, W)
        HW, cd = H * W, self.cd
        with ops.defer_bumps():
            xF = self._image(F_, C, F_aff)
            joff, n_joff = self._predictor(xF, C, self.joff_head.heads[0])
            mask_a, mask_aff = self._tower(xF, C, self.mask_head)
            jloc_a, jloc_aff = self._tower(xF, C, self.jloc_head)
            afm_a, afm_aff = self._tower(xF, C, self.afm_head)
            mz, mz_aff = self._eca(afm_a, afm_aff, mask_a, mask_aff, self.a2m_att)
            jz, jz_aff = self._eca(afm_a, afm_aff, jloc_a, jloc_aff, self.a2j_att)
            tmp = torch.zeros((B * HW, _up32(C)), dtype=cd, device=F_.device)
            hip.affine_relu_mix(tmp, mask_a, mask_aff, HW, C, b=mz, aff_b=mz_aff)          # mask_feature + mask_att_feature
            mask, n_mask = self._predictor(self._image(tmp, C), C, self.mask_predictor)
            hip.affine_relu_mix(tmp, jloc_a, jloc_aff, HW, C, b=jz, aff_b=jz_aff)
            jloc, n_jloc = self._predictor(self._image(tmp, C), C, self.jloc_predictor)
            afm, n_afm = self._predictor(self._image(afm_a, C, afm_aff), C, self.afm_predictor)
            afm_cd = afm if cd == torch.float32 else hip.cast(afm, cd)
            ref_a, ref_aff = self._tower(self._image(afm_cd, n_afm), n_afm, self.refuse_conv)
            cat = torch.zeros((B * HW, 2 * _up32(C)), dtype=cd, device=F_.device)     # torch.cat((features, afm_conv), dim=1)
            hip.affine_relu_mix(cat, F_, F_aff, HW, C)
            hip.affine_relu_mix(cat[:, C:], ref_a, ref_aff, HW, C)
            fin_a, fin_aff = self._tower(self._image(cat, 2 * C), 2 * C, self.final_conv)
            self._rows = {"joff": joff, "jloc": jloc}      # the predictors' own token-major fp32 rows [R, 8] (p3_hisup_junctions reads either layout)
            return {"joff": self._nchw(joff, n_joff), "jloc": self._nchw(jloc, n_jloc), "mask": self._nchw(mask, n_mask),
                    "afm": self._nchw(afm, n_afm), "remask": self._nchw(fin_a, 2, fin_aff)}


# ================================================================================================ the whole model (inference)
LOSS_KEYS = ("loss_jloc", "loss_joff", "loss_mask", "loss_afm", "loss_remask")


class AnnotationEncoder:
    """model_hisup.py:66-120: list of per-image annotation dicts (junctions [n, 2] (x, y), juncs_tag [n] in {1, 2}, edges_positive [e, 2],
    mask [H, W], height, width, juncs_index, bbox) -> (targets, metas); targets = {jloc [B,1,H,W] int64, joff [B,2,H,W], mask [B,1,H,W],
    afmap [B,2,H,W]} on the annotations' device.  The attraction field is p3_afm (csrc/afm.hip)."""

    def __init__(self, cfg):
        self.target_h = cfg.experiment.encoder.in_height
        self.target_w = cfg.experiment.encoder.in_width

    def __call__(self, annotations):
        targets, metas = [], []
        for ann in annotations:
            t, m = self._process_per_image(ann)
            targets.append(t)
            metas.append(m)
        return {k: torch.stack([t[k] for t in targets]) for k in ("jloc", "joff", "mask", "afmap")}, metas

    def _process_per_image(self, ann):
        junctions = ann["junctions"]
        device = junctions.device
        height, width = int(ann["height"]), int(ann["width"])
        jmap = torch.zeros((height, width), device=device, dtype=torch.long)
        joff = torch.zeros((2, height, width), device=device, dtype=torch.float32)
        edges = ann["edges_positive"]
        if len(edges) == 0:
            afmap = torch.zeros((1, 2, height, width), device=device, dtype=torch.float32)
        else:
            lines = torch.cat((junctions[edges[:, 0]], junctions[edges[:, 1]]), dim=-1)
            shape_info = torch.tensor([[0, lines.size(0), height, width]], dtype=torch.int32, device=device)
            afmap, _ = hip.afm(lines, shape_info, height, width)
        xint, yint = junctions[:, 0].long(), junctions[:, 1].long()
        off_x = junctions[:, 0] - xint.float() - 0.5
        off_y = junctions[:, 1] - yint.float() - 0.5
        if len(junctions) and (xint.min() < 0 or xint.max() >= width or yint.min() < 0 or yint.max() >= height):
            raise ValueError('Junctions out of bound')
        jmap[yint, xint] = ann["juncs_tag"].to(jmap.dtype)
        joff[0, yint, xint] = off_x
        joff[1, yint, xint] = off_y
        meta = {"junc": junctions, "junc_index": ann["juncs_index"], "bbox": ann["bbox"]}
        return {"jloc": jmap[None], "joff": joff, "mask": ann["mask"].float()[None], "afmap": afmap[0]}, meta


class EncoderDecoder(HiSupHeads):
    """model_hisup.py:122-308, inference: encoder + head set (`HiSupHeads` is the base class, so the state_dict is the reference's: `encoder.*`
    and the head keys at the top level) + what `forward_val` does after the heads, on the device: validation losses (p3_hisup_val_loss),
    junctions (p3_hisup_junctions), building regions (p3_hisup_regions) and, with polygons=True, the outer polygon of every region (p3_hisup_polygons,
    `get_poly_crowdai`), with inner_rings=True also the inner rings of its holes (p3_hisup_polygons_rings); see INTEGRATION.md for the order of sibling holes."""

    def __init__(self, cfg, encoder, max_regions=1024):
        super().__init__(cfg)
        self.cfg = cfg
        self.annotation_encoder = AnnotationEncoder(cfg)
        self.encoder = encoder
        enc = cfg.experiment.encoder
        self.pred_height, self.pred_width = int(enc.out_feature_height), int(enc.out_feature_width)
        self.origin_height, self.origin_width = int(enc.in_height), int(enc.in_width)
        self.max_regions = int(max_regions)

    def init_loss_dict(self):
        return {k: 0.0 for k in LOSS_KEYS}

    def forward(self, x_images, x_points, y=None):
        if self.training:
            return self.forward_train(x_images, x_points, y=y)
        return self.forward_val(x_images, x_points, y=y)

    def forward_train(self, x_images, x_lidar, y=None):
        raise NotImplementedError("HiSup training is not implemented on the HIP path: the head set has no backward yet. "
                                  "Call model.eval() and use forward_val / forward_val_device.")

    @torch.no_grad()
    def forward_common(self, x_images, x_lidar, y=None):
        """-> (targets | None, dict(joff, jloc, mask, afm, remask) NCHW fp32).  A `*_vit_cnn` encoder hands its token-major map with the pending
        BatchNorm + ReLU straight to the heads; any other encoder module is called for its NCHW map as in the reference (:201-208)."""
        targets = self.annotation_encoder(y)[0] if y is not None else None
        enc = self.cfg.experiment.encoder
        if not (enc.use_images or enc.use_lidar):
            raise ValueError("At least one of use_images or use_lidar must be True")
        if hasattr(self.encoder, "features_nhwc"):
            tokens = self.encoder.tokens(x_images if enc.use_images else None, x_lidar if enc.use_lidar else None)
            buf, sc, sh = self.encoder.features_nhwc(tokens)
            B, H = tokens.shape[0], self.encoder.out_size
            return targets, self._heads(buf, (sc, sh), B, H, H)
        if enc.use_images and enc.use_lidar:
            features = self.encoder(x_images, x_lidar)
        else:
            features = self.encoder(x_images if enc.use_images else x_lidar)
        return targets, HiSupHeads.forward(self, features)

    @torch.no_grad()
    def forward_val_device(self, x_images, x_lidar, y=None, polygons=False, inner_rings=False):
        """`forward_val` without any host synchronisation: -> (output, loss_dict) of device tensors.  output: juncs [B,600,2], junc_scores [B,600],
        junc_index [B,600], junc_counts [B,2] (hip.hisup_junctions), mask [B,H,W], regions = dict(labels, n_regions, area, bbox, score, status)
        (hip.hisup_regions_device; status[b] = 1: more than max_regions regions in image b) and `heads`, the five NCHW maps.  polygons=True adds
        output["polygons"], the dict of hip.hisup_polygons_device (outer polygons; a region with holes is flagged, its inner rings are not built) or, with
        inner_rings=True, the dict of hip.hisup_polygon_rings_device (the same outer polygons and the rings of the holes)."""
        targets, heads = self.forward_common(x_images, x_lidar, y)
        B, _, H, W = heads["joff"].shape
        assert H == self.pred_height and W == self.pred_width
        if (self.origin_height, self.origin_width) != (H, W):
            raise NotImplementedError(f"forward_val resizes the {H} x {W} mask to the input size {self.origin_height} x {self.origin_width} with "
                                      "cv2.resize; every shipped HiSup configuration predicts at the input size (224), so only ratio 1 is supported")
        loss_dict = self.init_loss_dict()
        if targets is not None:
            losses = hip.hisup_val_loss(heads["jloc"], heads["joff"], heads["mask"], heads["afm"], heads["remask"], targets["jloc"], targets["joff"],
                                        targets["mask"], targets["afmap"])
            loss_dict = {k: losses[i] for i, k in enumerate(LOSS_KEYS)}
        rows = self._rows
        juncs, scores, index, counts = hip.hisup_junctions(rows["jloc"], rows["joff"], self.origin_width / W, self.origin_height / H, shape=(B, H, W))
        reg = hip.hisup_regions_device(heads["remask"], self.max_regions)
        output = {"juncs": juncs, "junc_scores": scores, "junc_index": index, "junc_counts": counts, "mask": reg.pop("mask"), "regions": reg,
                  "heads": heads}
        if polygons:
            build = hip.hisup_polygon_rings_device if inner_rings else hip.hisup_polygons_device
            output["polygons"] = build(reg["labels"], reg["n_regions"], reg["bbox"], juncs, counts)
        return output, loss_dict

    @torch.no_grad()
    def forward_val(self, x_images, x_lidar, y=None, polygons=False, inner_rings=False):
        """model_hisup.py:229-293: -> (output, loss_dict).  output["juncs_pred"]: list of [n, 2] fp32 numpy arrays (x, y), class 2 first;
        output["mask_pred"]: list of [H, W] fp32 numpy arrays; output["regions"]: per image dict(labels int32 [H, W], area int32 [n], bbox int32 [n, 4],
        score fp32 [n]).  One device-to-host copy per kind.  polygons=True adds the reference's `polys_pred` (per image a list of closed float64 [k+1, 2]
        arrays (x, y), one per region that has a polygon, in label order) and `scores` (per image the matching regions' scores), and `poly_flags` (per image
        int32 [n]: bit 0 junction polygon, bit 1 the region has holes, bit 2 no polygon).  Only OUTER polygons are built: for a region with bit 1 the
        reference may add inner rings.  polygons=True with inner_rings=True builds them too: `polys_pred[b][i]` is what `get_poly_crowdai` returns, the outer
        polygon followed by the region's kept rings (those of holes with a border area of at least 50, in raster order of the holes' first cells), each
        closed, in one float64 [k, 2] array, and `poly_parts[b][i]` lists the length of each part (the reference's `edge_index`).  A ring in which the
        simplification keeps nothing is left out."""
        out, loss_dict = self.forward_val_device(x_images, x_lidar, y, polygons=polygons, inner_rings=inner_rings)
        reg = out["regions"]
        status, n_reg = reg["status"].cpu().numpy(), reg["n_regions"].cpu().numpy()
        if status.any():
            raise hip.P3Error(f"forward_val: an image has more than max_regions = {self.max_regions} regions (n_regions = {n_reg.tolist()})")
        juncs, counts = out["juncs"].cpu().numpy(), out["junc_counts"].cpu().numpy()
        mask, labels = out["mask"].cpu().numpy(), reg["labels"].cpu().numpy()
        area, bbox, score = reg["area"].cpu().numpy(), reg["bbox"].cpu().numpy(), reg["score"].cpu().numpy()
        B = mask.shape[0]
        output = {"juncs_pred": [juncs[b, :counts[b].sum()].copy() for b in range(B)], "mask_pred": [mask[b] for b in range(B)],
                  "regions": [{"labels": labels[b], "area": area[b, :n_reg[b]].copy(), "bbox": bbox[b, :n_reg[b]].copy(),
                               "score": score[b, :n_reg[b]].copy()} for b in range(B)]}
        if polygons:
            checked = hip.hisup_polygon_rings_checked if inner_rings else hip.hisup_polygons_checked
            pg = checked(dict(out["polygons"]), "forward_val(polygons=True)")
            pos, sl, flags = pg["pos"].cpu().numpy().astype("float64"), pg["poly_slice"].cpu().numpy(), pg["poly_flags"].cpu().numpy()
            output["polys_pred"] = [[pos[sl[b, i, 0]:sl[b, i, 1]] for i in range(n_reg[b]) if not flags[b, i] & 4] for b in range(B)]
            if inner_rings:
                rpos, rsl = pg["ring_pos"].cpu().numpy().astype("float64"), pg["ring_slice"].cpu().numpy()
                rflags, rr = pg["ring_flags"].cpu().numpy(), pg["region_rings"].cpu().numpy()
                output["poly_parts"] = []
                for b in range(B):
                    regions = [i for i in range(n_reg[b]) if not flags[b, i] & 4]
                    parts = [[poly] + [rpos[rsl[q, 0]:rsl[q, 1]] for q in range(rr[b, i, 0], rr[b, i, 1]) if not rflags[q] & 4]
                             for poly, i in zip(output["polys_pred"][b], regions)]
                    output["polys_pred"][b] = [np.concatenate(p) for p in parts]
                    output["poly_parts"].append([[len(x) for x in p] for p in parts])
            output["scores"] = [score[b, :n_reg[b]][(flags[b, :n_reg[b]] & 4) == 0].copy() for b in range(B)]
            output["poly_flags"] = [flags[b, :n_reg[b]].copy() for b in range(B)]
        return output, loss_dict


class HiSupModel(torch.nn.Module):
    """Factory with the reference's signature and encoder dispatch (model_hisup.py:312-360)."""

    def __new__(cls, cfg, local_rank=0):
        enc = cfg.experiment.encoder
        if enc.use_images and enc.use_lidar:
            if enc.name == "early_fusion_vit_cnn":
                encoder = EarlyFusionViTCNN(cfg, local_rank=local_rank)
            else:
                raise NotImplementedError(f"Encoder {enc.name} not implemented for {cls.__name__}")
        elif enc.use_images:
            if enc.name == "vit_cnn":
                encoder = ViTCNN(cfg, local_rank=local_rank)
            else:
                raise NotImplementedError(f"Encoder {enc.name} not implemented for {cls.__name__}")
        elif enc.use_lidar:
            if enc.name == "pointpillars_vit_cnn":
                encoder = PointPillarsViTCNN(cfg, local_rank=local_rank)
            else:
                raise NotImplementedError(f"Encoder {enc.name} not implemented for {cls.__name__}")
        else:
            raise ValueError("Please specify either and image or lidar encoder with encoder=<name>. See help for a list of available encoders.")
        model = EncoderDecoder(encoder=encoder, cfg=cfg)
        model.to(cfg.host.device)
        if cfg.host.multi_gpu:
            raise NotImplementedError("HiSupModel: multi_gpu wraps the model for training (SyncBatchNorm + DDP); the HIP path has HiSup inference only")
        return model
