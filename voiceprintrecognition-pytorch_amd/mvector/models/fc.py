"""The training-time classifier head: embedding [B, D] -> {'features', 'logits'} for the losses of ``mvector.loss``.

``num_blocks`` dense layers (a 1 x 1 convolution without bias and a BatchNorm1d, D -> ``inter_dim``) come first.  ``classifier_type``
'Cosine' then multiplies the L2-normalised rows with the L2-normalised class weights -- ``weight`` [num_speakers * K, D], K sub-centres per
speaker for ``SubCenterLoss`` -- so the logits are cosines; 'Linear' is an ordinary ``nn.Linear`` to ``num_speakers`` (``output``).  The
parameter names (``weight``, ``output.*``, ``blocks.<i>.linear.weight``, ``blocks.<i>.nonlinear.batchnorm.*``) are the reference's, so its
checkpoints load.  A plain torch module: the classifier GEMM is not part of the native path, the loss behind it is.

``mvector.models.SpeakerIdentification`` is still the stub that ``build_model`` refuses; import the class from here."""
import torch
import torch.nn.functional as F
from torch import nn


def get_nonlinear(config_str, channels):
    """'batchnorm-relu' and the like -> nn.Sequential of the named layers ('relu', 'prelu', 'batchnorm', 'batchnorm_' = without affine)"""
    makers = {'relu': lambda: nn.ReLU(inplace=True), 'prelu': lambda: nn.PReLU(channels), 'batchnorm': lambda: nn.BatchNorm1d(channels),
              'batchnorm_': lambda: nn.BatchNorm1d(channels, affine=False)}
    layers = nn.Sequential()
    for name in config_str.split('-'):
        if name not in makers:
            raise ValueError(f'Unexpected module ({name}).')
        layers.add_module(name.rstrip('_'), makers[name]())
    return layers


class DenseLayer(nn.Module):
    def __init__(self, in_channels, out_channels, bias=False, config_str='batchnorm-relu'):
        super().__init__()
        self.linear = nn.Conv1d(in_channels, out_channels, 1, bias=bias)
        self.nonlinear = get_nonlinear(config_str, out_channels)

    def forward(self, x):
        if x.dim() == 2:
            return self.nonlinear(self.linear(x.unsqueeze(-1)).squeeze(-1))
        return self.nonlinear(self.linear(x))


class SpeakerIdentification(nn.Module):
    def __init__(self, input_dim, num_speakers, classifier_type='Cosine', K=1, num_blocks=0, inter_dim=512):
        super().__init__()
        self.classifier_type = classifier_type
        self.blocks = nn.ModuleList()
        for _ in range(num_blocks):
            self.blocks.append(DenseLayer(input_dim, inter_dim, config_str='batchnorm'))
            input_dim = inter_dim
        if classifier_type == 'Cosine':
            self.weight = nn.Parameter(torch.empty(num_speakers * K, input_dim))
            nn.init.xavier_uniform_(self.weight)
        elif classifier_type == 'Linear':
            self.output = nn.Linear(input_dim, num_speakers)
        else:
            raise ValueError(f'不支持该输出层：{classifier_type}')

    def forward(self, features):
        x = features
        for block in self.blocks:
            x = block(x)
        if self.classifier_type == 'Cosine':
            logits = F.linear(F.normalize(x), F.normalize(self.weight))
        else:
            logits = self.output(x)
        return {'features': features, 'logits': logits}
