"""HiSup training losses - the five lines of `EncoderDecoder.forward_train` (pixelspointspolygons/models/hisup/model_hisup.py:302-306, with
`sigmoid_l1_loss` :27-37) and the weighted sum of `LossReducer` (train/trainer_hisup.py:31-39), on ONE fused HIP forward + gradient call
(`p3_hisup_train_loss`, csrc/hisup_loss.hip).

    criterion = HiSupCriterion(cfg)                       # weights: cfg.experiment.model.loss_weights, as LossReducer(cfg)
    total, loss_dict = criterion(heads, targets)          # heads: dict(joff, jloc, mask, afm, remask), targets: what AnnotationEncoder returns
    total.backward()

`total` carries the gradient with respect to the five head maps (the values and d total / d map come out of the same kernels); `loss_dict` holds the
five un-weighted losses under the reference's keys as detached device scalars, what the reference's trainer logs.  Any differentiable producer of the
five maps can train against it.  The head set of this package has no backward yet: `EncoderDecoder.forward_train` still raises, and `forward_common`
returns maps that require no gradient, for which the criterion computes the values alone.
"""
import torch

from . import hip
from .hisup import LOSS_KEYS

HEAD_KEYS = ("jloc", "joff", "mask", "afm", "remask")            # the maps in the order of the losses they enter (LOSS_KEYS)


@hip.precision_scoped
class _HiSupLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, jloc, joff, mask, afm, remask, t_jloc, t_joff, t_mask, t_afm, weights):
        preds = (jloc, joff, mask, afm, remask)
        need = any(ctx.needs_input_grad[:5])
        losses, grads = hip.hisup_train_loss(*[p.detach() for p in preds], t_jloc, t_joff, t_mask, t_afm, weights, need_grad=need)
        if need:
            ctx.save_for_backward(*grads)
        ctx.shapes = [(p.shape, p.dtype) for p in preds]
        ctx.mark_non_differentiable(losses)
        return losses[5].clone(), losses

    @staticmethod
    def backward(ctx, g, _g_losses):
        out = [(d * g).view(shape).to(dtype) if need else None
               for d, (shape, dtype), need in zip(ctx.saved_tensors, ctx.shapes, ctx.needs_input_grad[:5])]
        return (*out, None, None, None, None, None)


class HiSupCriterion(torch.nn.Module):
    """model_hisup.py:302-306 + LossReducer (trainer_hisup.py:31-39): `criterion(heads, targets)` -> (total, loss_dict)."""

    def __init__(self, cfg):
        super().__init__()
        lw = dict(cfg.experiment.model.loss_weights)
        missing = [k for k in LOSS_KEYS if k not in lw]
        if missing or len(lw) != len(LOSS_KEYS):
            raise ValueError(f"HiSupCriterion: loss_weights must hold exactly {LOSS_KEYS}, got {sorted(lw)}")
        self.loss_weights = {k: float(lw[k]) for k in LOSS_KEYS}

    @property
    def weights(self):
        """the five weights in LOSS_KEYS order, as the kernel takes them"""
        return [self.loss_weights[k] for k in LOSS_KEYS]

    def forward(self, heads, targets):
        for k in HEAD_KEYS:
            if heads[k].dim() != 4 or heads[k].dtype != torch.float32:
                raise hip.P3Error(f"HiSupCriterion: heads['{k}'] must be an NCHW fp32 map, got {tuple(heads[k].shape)} {heads[k].dtype}")
        total, losses = _HiSupLossFn.apply(*[heads[k] for k in HEAD_KEYS], targets["jloc"], targets["joff"], targets["mask"], targets["afmap"],
                                           self.weights)
        return total, {k: losses[i] for i, k in enumerate(LOSS_KEYS)}
