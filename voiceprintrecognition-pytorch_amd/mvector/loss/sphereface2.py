"""SphereFace2: a binary (one-vs-all) classification loss over every column of the cosine matrix, with a learnable bias.

With g(c) = 2 ((c + 1) / 2)^t - 1 bending the cosine, every column is a logistic loss: the target column as a positive with weight
``lanbuda`` and the margin against it, every other column as a negative with weight 1 - ``lanbuda`` and the margin for it.  ``margin_type``
'C' subtracts / adds the margin to g(c) (CosFace style), 'A' moves the angle by the margin before g (ArcFace style).  The row sums are
averaged over the batch.

Two paths, no fallback between them: 2-D CUDA logits of fp32 / fp16 / bf16 with the bias on the same device run ``_hip.sphereface2_forward`` /
``sphereface2_backward`` (csrc/sphereface2.hip: one streaming read forward, a read and a write backward; 16-bit logits are converted to fp32 on
load and everything after that is fp32 or fp64; the bias is read on the device, its gradient comes back with shape [1, 1]); every other tensor
runs the torch expression below.  After a native forward ``self.pred`` holds the int32 argmax of the cosines per row; on the torch path it is
None.  ``update(margin)`` takes effect at the next call (the native path carries its parameters per call)."""
import math

import torch
import torch.nn.functional as F
from torch import nn

from .softmax_family import _NATIVE_DTYPES


class _NativeSphereFace2Grad(torch.autograd.Function):
    """the closed-form gradients as a node of their own, so that a backward THROUGH them (create_graph=True) is refused by name"""

    @staticmethod
    def forward(ctx, grad_loss, logits, labels, bias, saved, params):
        from mvector import _hip
        grad, bias_grad = _hip.sphereface2_backward(logits, labels, bias, saved, grad_loss, **params)
        return grad, bias_grad.reshape(bias.shape)

    @staticmethod
    def backward(ctx, *_):
        raise RuntimeError('mvector.loss: the fused SphereFace2 loss has no second derivative (its gradient is a closed form without a graph); '
                           'fp64 or CPU logits run the torch expression, which has one')


class _NativeSphereFace2(torch.autograd.Function):
    """loss = mean over the batch of the row sums: forward and backward are one native call each"""

    @staticmethod
    def forward(ctx, logits, bias, labels, params):
        from mvector import _hip
        if logits.shape[1] > 1 and logits.stride(1) != 1:
            logits = logits.contiguous()
        loss, _, pred, saved = _hip.sphereface2_forward(logits, labels, bias, **params)
        ctx.save_for_backward(logits, labels, bias, saved)
        ctx.params = params
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    def backward(ctx, grad_loss, _grad_pred):
        logits, labels, bias, saved = ctx.saved_tensors
        grad, bias_grad = _NativeSphereFace2Grad.apply(grad_loss, logits, labels, bias, saved, ctx.params)
        return grad, bias_grad, None, None


class SphereFace2(nn.Module):
    def __init__(self, margin=0.2, scale=32.0, lanbuda=0.7, t=3, margin_type='C'):
        super().__init__()
        self.scale = scale
        self.bias = nn.Parameter(torch.zeros(1, 1))
        self.t = t
        self.lanbuda = lanbuda
        self.margin_type = margin_type
        self.pred = None
        self.update(margin)

    def update(self, margin=0.2):
        self.margin = margin
        self.cos_m, self.sin_m = math.cos(margin), math.sin(margin)
        self.th = math.cos(math.pi - margin)
        self.mmm = 1.0 + math.cos(math.pi - margin)

    def fun_g(self, z, t: int):
        return 2 * torch.pow((z + 1) / 2, t) - 1

    def forward(self, inputs, labels):
        """inputs: {'features': [B, D], 'logits': [B, N]}, labels [B] -> the scalar loss"""
        cos = inputs['logits']
        if cos.is_cuda and cos.dim() == 2 and cos.dtype in _NATIVE_DTYPES and self.bias.device == cos.device and self.bias.dtype == torch.float32:
            params = dict(margin=self.margin, scale=self.scale, lanbuda=self.lanbuda, t=self.t, margin_type=self.margin_type)
            loss, self.pred = _NativeSphereFace2.apply(cos, self.bias, labels, params)
            return loss
        self.pred = None
        return self.torch_expression(inputs, labels)

    def torch_expression(self, inputs, labels):
        """the loss as a differentiable torch expression in the logits' dtype, on any device (what every non-native tensor runs)"""
        cos = inputs['logits']
        bias = self.bias[0][0]
        if self.margin_type == 'A':
            sin = torch.sqrt(1.0 - cos * cos)
            toward = torch.where(cos > self.th, cos * self.cos_m - sin * self.sin_m, cos - self.mmm)   # cos(theta + m), continued past pi
            away = cos * self.cos_m + sin * self.sin_m                                                  # cos(theta - m)
            pos_logit = self.scale * self.fun_g(toward, self.t) + bias
            neg_logit = self.scale * self.fun_g(away, self.t) + bias
        else:
            bent = self.fun_g(cos, self.t)
            pos_logit = self.scale * (bent - self.margin) + bias
            neg_logit = self.scale * (bent + self.margin) + bias
        as_positive = self.lanbuda * torch.log(1 + torch.exp(-pos_logit))
        as_negative = (1 - self.lanbuda) * torch.log(1 + torch.exp(neg_logit))
        is_target = F.one_hot(labels.long(), cos.shape[1]).to(cos.dtype)
        return (is_target * as_positive + (1 - is_target) * as_negative).sum(dim=1).mean()
