"""ResNetSE with the reference's constructor and state_dict layout (mvector/models/resnet_se.py:7-145).

The parameter tree (``conv1, bn1, layer{1..4}.{j}.{conv1,bn1,conv2,bn2,conv3,bn3,se.fc.{0,2},downsample.{0,1}}``, ``pooling.*``,
``bn2``, ``linear``, ``bn3``) is the reference's, so its ``model.pth`` loads unchanged.  Eval-mode CUDA forwards run on the native
handle (csrc/resnet_se.hip: every conv + BatchNorm + ReLU is one conv2ds launch on S16 maps, the SE layer and the hand-over to the
pooling head are the kernels of csrc/se2d.hip); the torch forward below serves CPU tensors, training-mode calls and forwards that
need input gradients.

``mvector.models.build_model`` still refuses the name 'ResNetSE' (its registry entry is the stub one test pins): import the class
from this module, as the reference allows as well.
"""
import torch.nn as nn

from mvector.models._native import NativeBackbone
from mvector.models.pooling import AttentiveStatisticsPooling, SelfAttentivePooling, TemporalAveragePooling, TemporalStatisticsPooling

__all__ = ['ResNetSE', 'SEBottleneck', 'SELayer']


class SELayer(nn.Module):
    """Squeeze (mean over the map) and excitation (two dense layers, sigmoid): a gate per channel."""

    def __init__(self, channel, reduction=8):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(nn.Linear(channel, channel // reduction), nn.ReLU(inplace=True),
                                nn.Linear(channel // reduction, channel), nn.Sigmoid())

    def forward(self, x):
        b, c = x.shape[:2]
        return x * self.fc(self.avg_pool(x).view(b, c)).view(b, c, 1, 1)


class SEBottleneck(nn.Module):
    """1x1 -> 3x3 (stride) -> 1x1 (twice the planes) -> SE gate -> + residual -> ReLU."""
    expansion = 2

    def __init__(self, inplanes, planes, stride=1, downsample=None, reduction=8):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.se = SELayer(planes * self.expansion, reduction)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.se(self.bn3(self.conv3(out)))
        residual = x if self.downsample is None else self.downsample(x)
        return self.relu(out + residual)


_POOLINGS = {'ASP': (lambda c: AttentiveStatisticsPooling(c, attention_channels=128), 2), 'SAP': (lambda c: SelfAttentivePooling(c, 128), 1),
             'TAP': (lambda c: TemporalAveragePooling(), 1), 'TSP': (lambda c: TemporalStatisticsPooling(), 2)}


class ResNetSE(NativeBackbone, nn.Module):
    _native_kind = 'resnet_se'

    def __init__(self, input_size, layers=[3, 4, 6, 3], num_filters=[32, 64, 128, 256], embd_dim=192, pooling_type='ASP'):
        super().__init__()
        self.inplanes = num_filters[0]
        self.embd_dim = embd_dim
        self._cfg = dict(input_size=input_size, layers=list(layers), num_filters=list(num_filters), pooling_type=pooling_type)
        self.conv1 = nn.Conv2d(1, num_filters[0], kernel_size=3, stride=(1, 1), padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(num_filters[0])
        self.relu = nn.ReLU(inplace=True)
        self.layer1 = self._make_layer(SEBottleneck, num_filters[0], layers[0])
        self.layer2 = self._make_layer(SEBottleneck, num_filters[1], layers[1], stride=(2, 2))
        self.layer3 = self._make_layer(SEBottleneck, num_filters[2], layers[2], stride=(2, 2))
        self.layer4 = self._make_layer(SEBottleneck, num_filters[3], layers[3], stride=(2, 2))
        cat_channels = num_filters[3] * SEBottleneck.expansion * (input_size // 8)
        if pooling_type not in _POOLINGS:
            raise Exception(f'没有{pooling_type}池化层！')
        make, mult = _POOLINGS[pooling_type]
        self.pooling = make(cat_channels)
        self.bn2 = nn.BatchNorm1d(cat_channels * mult)
        self.linear = nn.Linear(cat_channels * mult, embd_dim)
        self.bn3 = nn.BatchNorm1d(embd_dim)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        layers.extend(block(self.inplanes, planes) for _ in range(1, blocks))
        return nn.Sequential(*layers)

    def _native_supported(self):
        """what mv_resnetse_create refuses (csrc/resnet_se.hip), by name"""
        c = self._cfg
        if c['input_size'] < 8 or c['input_size'] % 8:
            return False, f"input_size={c['input_size']} (not a multiple of 8)"
        if len(c['num_filters']) != 4 or len(c['layers']) != 4:
            return False, 'a network that does not have four stages'
        bad = [f for f in c['num_filters'] if f < 16 or f % 16 or f > 512]
        if bad:
            return False, f"num_filters={c['num_filters']} (every entry must be a multiple of 16, at most 512)"
        if min(c['layers']) < 1:
            return False, f"layers={c['layers']} (a stage without blocks)"
        if type(self.layer1[0]) is not SEBottleneck:
            return False, 'a custom block class'
        return True, ''

    def _native_cfg(self):
        from mvector import _hip
        c = self._cfg
        cfg = _hip.MvResNetSeCfg()
        cfg.input_size, cfg.embd_dim, cfg.reduction = c['input_size'], self.embd_dim, 8
        for i in range(4):
            cfg.layers[i], cfg.num_filters[i] = c['layers'][i], c['num_filters'][i]
        cfg.pooling_type = _hip.POOLING_TYPES[c['pooling_type']]
        return cfg

    def forward(self, x):
        """x: (B, T, F) -> (B, embd_dim)."""
        if self._use_native(x):
            return self._native_forward(x)
        x = self.relu(self.bn1(self.conv1(x.transpose(2, 1).unsqueeze(1))))   # (B,T,F) => (B,1,F,T)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = self.pooling(x.reshape(x.shape[0], -1, x.shape[-1]))
        return self.bn3(self.linear(self.bn2(x)))
