"""The softmax family of classification losses: cross-entropy over margin-adjusted logits.

With ``c_j`` the cosine of class j (for ``K`` sub-centres the largest of the class's K columns), ``y`` the label and ``s`` the scale:

    CELoss          z_j = c_j
    AMLoss          z_j = s c_j,  z_y = s (c_y - m)                               (additive margin)
    ARMLoss         the AM values; every z_j below z_y is replaced by 0           (additive real margin)
    AAMLoss         z_j = s c_j,  z_y = s cos(theta_y + m) while theta_y + m stays below pi (c_y > cos(pi - m)), else s (c_y - 1 - cos(pi - m));
                    with ``easy_margin`` the margin applies only where c_y > 0    (additive angular margin)
    SubCenterLoss   AAMLoss over the sub-centre maxima

and the loss is the mean over the batch of the cross-entropy of z with label smoothing.  ``update(margin)`` is the margin scheduler's hook: it
takes effect at the next call (the native path carries its parameters per call).

Two paths, no fallback between them: 2-D CUDA logits of fp32 / fp16 / bf16 run ``_hip.margin_ce_forward`` / ``margin_ce_backward`` (16-bit
logits are converted to fp32 on load and everything after that is fp32 or fp64 -- more exact than evaluating the expression in the logits'
dtype); every other tensor runs ``margin_logits`` + ``F.cross_entropy``.  After a native forward ``self.pred`` holds the int32 argmax of the
cosines per row (what an accuracy needs), computed in the same pass."""
import math

import torch
import torch.nn.functional as F
from torch import nn

_NATIVE_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _angular_constants(margin):
    return dict(cos_m=math.cos(margin), sin_m=math.sin(margin), th=math.cos(math.pi - margin), mmm=1.0 + math.cos(math.pi - margin))


def margin_logits(logits, labels, kind, margin=0.2, scale=32.0, easy_margin=False, K=1):
    """[B, N * K] logits -> the [B, N] matrix z the cross-entropy is taken of, as a differentiable torch expression in the logits' dtype"""
    B = logits.shape[0]
    cos = logits if K == 1 else logits.reshape(B, logits.shape[1] // K, K).max(dim=2).values
    if kind == 'ce':
        return cos
    index = labels.reshape(B, 1).long()
    cos_y = cos.gather(1, index)
    if kind in ('am', 'arm'):
        # the margin is a float32 quantity whatever the logits' dtype: the reference writes it into a float32 tensor
        m = torch.tensor(margin, dtype=torch.float32).to(device=cos.device, dtype=cos.dtype if cos.dtype == torch.float64 else torch.float32)
        z_y = scale * (cos_y - m)
    else:
        k = _angular_constants(margin)
        sin_y = torch.sqrt(1.0 - cos_y * cos_y)
        with_margin = cos_y * k['cos_m'] - sin_y * k['sin_m']
        if easy_margin:
            z_y = torch.where(cos_y > 0, with_margin, cos_y) * scale
        else:
            z_y = torch.where(cos_y > k['th'], with_margin, cos_y - k['mmm']) * scale
    is_target = torch.zeros_like(cos, dtype=torch.bool).scatter_(1, index, True)
    z = torch.where(is_target, z_y.to(cos.dtype), scale * cos)
    if kind == 'arm':
        z = torch.where((z - z_y).detach() < 0, torch.zeros_like(z), z)
    return z


class _NativeMarginCEGrad(torch.autograd.Function):
    """the closed-form gradient as a node of its own, so that a backward THROUGH it (create_graph=True) is refused by name"""

    @staticmethod
    def forward(ctx, grad_loss, logits, labels, saved, params):
        from mvector import _hip
        return _hip.margin_ce_backward(logits, labels, saved, grad_loss, **params)

    @staticmethod
    def backward(ctx, *_):
        raise RuntimeError('mvector.loss: the fused margin-softmax loss has no second derivative (its gradient is a closed form without a graph); '
                           'fp64 or CPU logits run the torch expression, which has one')


class _NativeMarginCE(torch.autograd.Function):
    """loss = mean cross-entropy of z(logits): forward and backward are one native call each"""

    @staticmethod
    def forward(ctx, logits, labels, params):
        from mvector import _hip
        if logits.shape[1] > 1 and logits.stride(1) != 1:
            logits = logits.contiguous()
        loss, _, pred, saved = _hip.margin_ce_forward(logits, labels, **params)
        ctx.save_for_backward(logits, labels, saved)
        ctx.params = params
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    def backward(ctx, grad_loss, _grad_pred):
        logits, labels, saved = ctx.saved_tensors
        return _NativeMarginCEGrad.apply(grad_loss, logits, labels, saved, ctx.params), None, None


class _SoftmaxFamilyLoss(nn.Module):
    kind = None

    def __init__(self, margin=0.2, scale=32, easy_margin=False, K=1, label_smoothing=0.0):
        super().__init__()
        self.margin = margin
        self.scale = scale
        self.easy_margin = easy_margin
        self.K = K
        self.label_smoothing = label_smoothing
        self.pred = None

    def _params(self):
        return dict(kind=self.kind, margin=self.margin, scale=self.scale, easy_margin=self.easy_margin, K=self.K)

    def forward(self, inputs, labels):
        """inputs: {'features': [B, D], 'logits': [B, N * K]}, labels [B] -> the scalar loss"""
        logits = inputs['logits']
        if logits.is_cuda and logits.dim() == 2 and logits.dtype in _NATIVE_DTYPES:
            loss, self.pred = _NativeMarginCE.apply(logits, labels, dict(self._params(), label_smoothing=self.label_smoothing))
            return loss
        self.pred = None
        z = margin_logits(logits, labels, **self._params())
        return F.cross_entropy(z, labels.long(), label_smoothing=self.label_smoothing)

    def update(self, margin=0.2):
        self.margin = margin


class CELoss(_SoftmaxFamilyLoss):
    kind = 'ce'

    def __init__(self, label_smoothing=0.0):
        super().__init__(margin=0.0, scale=1.0, label_smoothing=label_smoothing)

    def update(self, margin=0.2):
        pass


class AMLoss(_SoftmaxFamilyLoss):
    kind = 'am'

    def __init__(self, margin=0.3, scale=32, label_smoothing=0.0):
        super().__init__(margin=margin, scale=scale, label_smoothing=label_smoothing)


class ARMLoss(_SoftmaxFamilyLoss):
    kind = 'arm'

    def __init__(self, margin=0.3, scale=32, label_smoothing=0.0):
        super().__init__(margin=margin, scale=scale, label_smoothing=label_smoothing)


class AAMLoss(_SoftmaxFamilyLoss):
    kind = 'aam'

    def __init__(self, margin=0.2, scale=32, easy_margin=False, label_smoothing=0.0):
        super().__init__(margin=margin, scale=scale, easy_margin=easy_margin, label_smoothing=label_smoothing)


class SubCenterLoss(_SoftmaxFamilyLoss):
    kind = 'subcenter'

    def __init__(self, margin=0.2, scale=32, easy_margin=False, K=3, label_smoothing=0.0):
        super().__init__(margin=margin, scale=scale, easy_margin=easy_margin, K=K, label_smoothing=label_smoothing)
