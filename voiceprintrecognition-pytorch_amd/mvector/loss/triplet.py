"""Triplet loss on angular margin with batch-hard mining, plus the plain cross-entropy of the logits.

Over the [B, B] cosine matrix of the (normalised) features every anchor takes its hardest positive (the least similar row of its own label,
itself included) and its hardest negative (the most similar row of another label); the ranking term is
mean(max(0, margin - (ap - an))), and with ``add_absolute`` the two similarities are also held against fixed values (``ap_value``,
``an_value``).

Two paths, no fallback between them: when features and logits are both 2-D CUDA tensors of fp32 / fp16 / bf16, the cross-entropy runs the native
function of ``softmax_family`` (kind 'ce' with the class's ``label_smoothing``; ``self.pred`` is its int32 argmax) and the triplet term runs
``_hip.triplet_forward`` / ``triplet_backward`` (csrc/triplet.hip: the features are upcast on load and everything after that is fp64, the [B, B]
matrix is never stored, the backward is a gather over the mined indices); the two fp32 scalars are added in torch.  Every other tensor runs the
torch expression below, and ``self.pred`` is None."""
import torch
import torch.nn.functional as F
from torch import nn

from .softmax_family import _NATIVE_DTYPES, _NativeMarginCE


class _NativeTripletGrad(torch.autograd.Function):
    """the gather as a node of its own, so that a backward THROUGH it (create_graph=True) is refused by name"""

    @staticmethod
    def forward(ctx, grad_loss, features, labels, mined, index, params):
        from mvector import _hip
        return _hip.triplet_backward(features, labels, mined, index, grad_loss, **params)

    @staticmethod
    def backward(ctx, *_):
        raise RuntimeError('mvector.loss: the fused triplet loss has no second derivative (its gradient is a closed form without a graph); '
                           'fp64 or CPU features run the torch expression, which has one')


class _NativeTriplet(torch.autograd.Function):
    """the ranking term and the two absolute terms: forward and backward are one native call each"""

    @staticmethod
    def forward(ctx, features, labels, params):
        from mvector import _hip
        if features.shape[1] > 1 and features.stride(1) != 1:
            features = features.contiguous()
        loss, mined, index = _hip.triplet_forward(features, labels, **params)
        ctx.save_for_backward(features, labels, mined, index)
        ctx.params = params
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        features, labels, mined, index = ctx.saved_tensors
        return _NativeTripletGrad.apply(grad_loss, features, labels, mined, index, ctx.params), None, None


class TripletAngularMarginLoss(nn.Module):
    def __init__(self, margin=0.5, normalize_feature=True, add_absolute=True, absolute_loss_weight=1.0, ap_value=0.8, an_value=0.4,
                 label_smoothing=0.0):
        super().__init__()
        self.margin = margin
        self.normalize_feature = normalize_feature
        self.add_absolute = add_absolute
        self.absolute_loss_weight = absolute_loss_weight
        self.ap_value = ap_value
        self.an_value = an_value
        self.label_smoothing = label_smoothing
        self.pred = None

    def update(self, margin=0.5):
        self.margin = margin

    def forward(self, inputs, labels):
        """inputs: {'features': [B, D], 'logits': [B, N]}, labels [B] -> the scalar loss"""
        features, logits = inputs['features'], inputs['logits']
        if all(x.is_cuda and x.dim() == 2 and x.dtype in _NATIVE_DTYPES for x in (features, logits)):
            ce, self.pred = _NativeMarginCE.apply(logits, labels, dict(kind='ce', margin=0.0, scale=1.0, easy_margin=False, K=1,
                                                                      label_smoothing=self.label_smoothing))
            params = dict(margin=self.margin, normalize=self.normalize_feature, add_absolute=self.add_absolute,
                          absolute_loss_weight=self.absolute_loss_weight, ap_value=self.ap_value, an_value=self.an_value)
            return _NativeTriplet.apply(features, labels, params) + ce
        self.pred = None
        return self.torch_expression(inputs, labels)

    def torch_expression(self, inputs, labels):
        """the loss as a differentiable torch expression in the tensors' dtype, on any device (what every non-native tensor runs)"""
        features, logits = inputs['features'], inputs['logits']
        ce = F.cross_entropy(logits, labels.long(), label_smoothing=self.label_smoothing)
        if self.normalize_feature:
            features = features / torch.norm(features, p=2, dim=-1, keepdim=True)
        sim = features @ features.t()
        same = labels.reshape(-1, 1) == labels.reshape(1, -1)
        ap = sim.masked_fill(~same, float('inf')).min(dim=1).values
        an = sim.masked_fill(same, float('-inf')).max(dim=1).values
        loss = torch.clamp(self.margin - (ap - an), min=0).mean()
        if self.add_absolute:
            short = self.ap_value - ap
            short = torch.where(short > 0, short, torch.zeros_like(short))
            over = an - self.an_value
            over = torch.where(over > 0, over, torch.ones_like(over))   # (a negative at or below an_value counts as 1, as in the reference)
            loss = (over.mean() + short.mean()) * self.absolute_loss_weight + loss
        return loss + ce
