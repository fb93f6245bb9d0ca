"""Triplet loss on angular margin with batch-hard mining, plus the plain cross-entropy of the logits.

Over the [B, B] cosine matrix of the (normalised) features every anchor takes its hardest positive (the least similar row of its own label,
itself included) and its hardest negative (the most similar row of another label); the ranking term is
mean(max(0, margin - (ap - an))), and with ``add_absolute`` the two similarities are also held against fixed values (``ap_value``,
``an_value``).  Runs as a torch expression on every device (a native kernel is the named follow-up)."""
import torch
import torch.nn.functional as F
from torch import nn


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

    def update(self, margin=0.5):
        self.margin = margin

    def forward(self, inputs, labels):
        """inputs: {'features': [B, D], 'logits': [B, N]}, labels [B] -> the scalar loss"""
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
