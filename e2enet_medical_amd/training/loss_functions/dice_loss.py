"""Dice + cross-entropy loss on the fused HIP kernels.

Drop-in for reference e2enet/training/loss_functions/dice_loss.py ``DC_and_CE_loss`` (:302-359) in the configuration
the trainer builds (nnUNetTrainer_simple.py:100): SoftDiceLoss(softmax, batch_dice, do_bg=False, smooth=1e-5) +
RobustCrossEntropyLoss, aggregate="sum", unit weights.  Forward and backward are the two kernels
``e2e_dc_ce_reduce`` / ``e2e_dc_ce_grad``; the module is an autograd node so it also composes with the reference's
``MultipleOutputLoss2``.

``DC_and_BCE_loss`` (:362-387) is the loss of the region trainer (nnUNetTrainerV2BraTSRegions): BCEWithLogitsLoss() +
SoftDiceLoss(sigmoid, batch_dice, do_bg=True, smooth) over multi-hot region targets, on ``e2e_dc_bce_reduce`` /
``e2e_dc_bce_grad``.
"""
import torch
from torch import nn

from ..._lib import lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _DcCeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, batch_dice, smooth):
        if not logits.is_cuda:
            raise RuntimeError("DC_and_CE_loss (MI355X) needs GPU tensors: there is no CPU fallback")
        logits = logits.contiguous().float()
        target = target.contiguous().float()
        b, k = logits.shape[:2]
        spatial = logits[0, 0].numel()
        ws = torch.empty(lib().loss_ws_bytes(b, k) // 8, dtype=torch.float64, device=logits.device)
        dl = torch.empty_like(logits)
        loss = torch.zeros(1, dtype=torch.float32, device=logits.device)
        lib().dc_ce_reduce(logits.data_ptr(), target.data_ptr(), ws.data_ptr(), b, k, spatial, _stream())
        lib().dc_ce_grad(logits.data_ptr(), target.data_ptr(), ws.data_ptr(), 1.0, 1 if batch_dice else 0, float(smooth),
                         dl.data_ptr(), loss.data_ptr(), b, k, spatial, _stream())
        ctx.save_for_backward(dl)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None, None, None


class DC_and_CE_loss(nn.Module):
    def __init__(self, soft_dice_kwargs, ce_kwargs, aggregate="sum", square_dice=False, weight_ce=1, weight_dice=1,
                 log_dice=False, ignore_label=None):
        super().__init__()
        if square_dice or log_dice or ignore_label is not None or weight_ce != 1 or weight_dice != 1 or aggregate != "sum" \
                or ce_kwargs:
            raise NotImplementedError("fused DC_and_CE_loss implements the trainer's configuration only "
                                      "(nnUNetTrainer_simple.py:100)")
        if soft_dice_kwargs.get('do_bg', True):
            raise NotImplementedError("fused DC_and_CE_loss implements do_bg=False")
        self.batch_dice = bool(soft_dice_kwargs.get('batch_dice', False))
        self.smooth = float(soft_dice_kwargs.get('smooth', 1.))

    def forward(self, net_output, target):
        return _DcCeFunction.apply(net_output, target, self.batch_dice, self.smooth)


class _DcBceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, batch_dice, smooth):
        if not logits.is_cuda:
            raise RuntimeError("DC_and_BCE_loss (MI355X) needs GPU tensors: there is no CPU fallback")
        logits = logits.contiguous().float()
        target = target.contiguous().float()
        if tuple(target.shape) != tuple(logits.shape):
            raise ValueError("DC_and_BCE_loss takes multi-hot targets of the logits' shape %s, got %s"
                             % (tuple(logits.shape), tuple(target.shape)))
        b, r = logits.shape[:2]
        spatial = logits[0, 0].numel()
        ws = torch.empty(lib().loss_ws_bytes(b, r) // 8, dtype=torch.float64, device=logits.device)
        dl = torch.empty_like(logits)
        loss = torch.zeros(1, dtype=torch.float32, device=logits.device)
        lib().dc_bce_reduce(logits.data_ptr(), target.data_ptr(), None, ws.data_ptr(), b, r, spatial, _stream())
        lib().dc_bce_grad(logits.data_ptr(), target.data_ptr(), None, ws.data_ptr(), 1.0, 1 if batch_dice else 0, float(smooth),
                          dl.data_ptr(), loss.data_ptr(), b, r, spatial, _stream())
        ctx.save_for_backward(dl)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None, None, None


class DC_and_BCE_loss(nn.Module):
    def __init__(self, bce_kwargs, soft_dice_kwargs, aggregate="sum"):
        """The network must not apply a nonlinearity: the kernels take logits.  Targets are multi-hot [B, R, ...] (what
        ConvertSegmentationToRegionsTransform yields); the engine's own path (Engine.loss_backward(regions=...)) takes the label
        map instead and gives the same numbers."""
        super().__init__()
        if bce_kwargs:
            raise NotImplementedError("fused DC_and_BCE_loss implements BCEWithLogitsLoss() without arguments, got %r" % (bce_kwargs,))
        if aggregate != "sum":
            raise NotImplementedError("fused DC_and_BCE_loss implements aggregate='sum'")
        if not soft_dice_kwargs.get('do_bg', True):
            raise NotImplementedError("fused DC_and_BCE_loss implements do_bg=True: every region has a dice term")
        unknown = set(soft_dice_kwargs) - {'batch_dice', 'do_bg', 'smooth'}
        if unknown:
            raise NotImplementedError("fused DC_and_BCE_loss does not implement SoftDiceLoss arguments %s" % sorted(unknown))
        self.aggregate = aggregate
        self.batch_dice = bool(soft_dice_kwargs.get('batch_dice', False))
        self.smooth = float(soft_dice_kwargs.get('smooth', 1.))

    def forward(self, net_output, target):
        return _DcBceFunction.apply(net_output, target, self.batch_dice, self.smooth)
