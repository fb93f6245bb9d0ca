"""SphereFace2: a binary (one-vs-all) classification loss over every column of the cosine matrix, with a learnable bias.

With g(c) = 2 ((c + 1) / 2)^t - 1 bending the cosine, every column is a logistic loss: the target column as a positive with weight
``lanbuda`` and the margin against it, every other column as a negative with weight 1 - ``lanbuda`` and the margin for it.  ``margin_type``
'C' subtracts / adds the margin to g(c) (CosFace style), 'A' moves the angle by the margin before g (ArcFace style).  The row sums are
averaged over the batch.  Runs as a torch expression on every device (a native kernel is the named follow-up)."""
import math

import torch
import torch.nn.functional as F
from torch import nn


class SphereFace2(nn.Module):
    def __init__(self, margin=0.2, scale=32.0, lanbuda=0.7, t=3, margin_type='C'):
        super().__init__()
        self.scale = scale
        self.bias = nn.Parameter(torch.zeros(1, 1))
        self.t = t
        self.lanbuda = lanbuda
        self.margin_type = margin_type
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
