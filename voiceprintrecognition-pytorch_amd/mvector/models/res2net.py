"""Res2Net with the reference's constructor and state_dict layout (mvector/models/res2net.py:10-174).

The parameter tree (``conv1, bn1, layer{1..4}.{j}.{conv1,bn1,convs.{i},bns.{i},conv3,bn3,downsample.{0,1}}``, ``pooling.*``, ``bn2``,
``linear``, ``bn3``) is the reference's, so its ``model.pth`` loads unchanged.  Eval-mode CUDA forwards run on the native handle
(csrc/res2net.hip: every 1x1 / 3x3 conv + BatchNorm + ReLU is one conv2ds launch on S16 maps; the 7x7 stem, the max-pool behind it and
the average pool of the 'stage' blocks are the kernels of csrc/res2net2d.hip); the torch forward below serves CPU tensors, training-mode
calls and forwards that need input gradients.

``mvector.models.build_model`` still refuses the name 'Res2Net' (its registry entry is the stub one test pins): import the class from
this module, as the reference allows as well.
"""
import math

import torch
import torch.nn as nn

from mvector.models._native import NativeBackbone
from mvector.models.pooling import AttentiveStatisticsPooling, SelfAttentivePooling, TemporalAveragePooling, TemporalStatisticsPooling

__all__ = ['Res2Net', 'Bottle2neck']


class Bottle2neck(nn.Module):
    """1x1 into ``scale`` slices of ``width`` channels -> a 3x3 conv per slice but the last ('normal': each reads the output of the one before
    plus its own slice; 'stage', the first block of a stage: each reads its own slice) -> the last slice passed on ('normal') or average-pooled
    ('stage') -> 1x1 (four times the planes) -> + residual -> ReLU."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, baseWidth=26, scale=4, stype='normal'):
        super().__init__()
        width = int(math.floor(planes * (baseWidth / 64.0)))
        self.conv1 = nn.Conv2d(inplanes, width * scale, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(width * scale)
        self.nums = 1 if scale == 1 else scale - 1
        if stype == 'stage':
            self.pool = nn.AvgPool2d(kernel_size=3, stride=stride, padding=1)
        self.convs = nn.ModuleList(nn.Conv2d(width, width, kernel_size=3, stride=stride, padding=1, bias=False) for _ in range(self.nums))
        self.bns = nn.ModuleList(nn.BatchNorm2d(width) for _ in range(self.nums))
        self.conv3 = nn.Conv2d(width * scale, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stype = stype
        self.scale = scale
        self.width = width

    def forward(self, x):
        spx = torch.split(self.relu(self.bn1(self.conv1(x))), self.width, 1)
        outs = []
        sp = None
        for i in range(self.nums):
            sp = spx[i] if i == 0 or self.stype == 'stage' else sp + spx[i]
            sp = self.relu(self.bns[i](self.convs[i](sp)))
            outs.append(sp)
        if self.scale != 1:
            outs.append(spx[self.nums] if self.stype == 'normal' else self.pool(spx[self.nums]))
        out = self.bn3(self.conv3(torch.cat(outs, 1)))
        residual = x if self.downsample is None else self.downsample(x)
        return self.relu(out + residual)


_POOLINGS = {'ASP': (lambda c: AttentiveStatisticsPooling(c, attention_channels=128), 2), 'SAP': (lambda c: SelfAttentivePooling(c, 128), 1),
             'TAP': (lambda c: TemporalAveragePooling(), 1), 'TSP': (lambda c: TemporalStatisticsPooling(), 2)}


def _frequency_sizes(input_size):
    """frequency size behind the stem, the max-pool and each of the four stages (layer1 keeps it)"""
    h = [(input_size - 5) // 3 + 1]
    h.append((h[-1] - 1) // 2 + 1)
    h.append(h[-1])
    for _ in range(3):
        h.append((h[-1] - 1) // 2 + 1)
    return h


class Res2Net(NativeBackbone, nn.Module):
    _native_kind = 'res2net'

    def __init__(self, input_size, m_channels=32, layers=[3, 4, 6, 3], base_width=32, scale=2, embd_dim=192, pooling_type='ASP'):
        super().__init__()
        self.inplanes = m_channels
        self.base_width = base_width
        self.scale = scale
        self.embd_dim = embd_dim
        self._cfg = dict(input_size=input_size, m_channels=m_channels, layers=list(layers), pooling_type=pooling_type)
        self.conv1 = nn.Conv2d(1, m_channels, kernel_size=7, stride=3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(m_channels)
        self.relu = nn.ReLU(inplace=True)
        self.max_pool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(Bottle2neck, m_channels, layers[0])
        self.layer2 = self._make_layer(Bottle2neck, m_channels * 2, layers[1], stride=2)
        self.layer3 = self._make_layer(Bottle2neck, m_channels * 4, layers[2], stride=2)
        self.layer4 = self._make_layer(Bottle2neck, m_channels * 8, layers[3], stride=2)
        cat_channels = m_channels * 8 * Bottle2neck.expansion * (input_size // base_width)
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
        layers = [block(self.inplanes, planes, stride, downsample=downsample, stype='stage', baseWidth=self.base_width, scale=self.scale)]
        self.inplanes = planes * block.expansion
        layers.extend(block(self.inplanes, planes, baseWidth=self.base_width, scale=self.scale) for _ in range(1, blocks))
        return nn.Sequential(*layers)

    def _native_supported(self):
        """what mv_res2net_create refuses (csrc/res2net.hip), by name"""
        c = self._cfg
        if len(c['layers']) != 4:
            return False, 'a network that does not have four stages'
        if not 1 <= self.scale <= 8:
            return False, f'scale={self.scale} (outside 1..8)'
        if c['m_channels'] < 8 or c['m_channels'] % 8 or c['m_channels'] > 256:
            return False, f"m_channels={c['m_channels']} (not a multiple of 8, or above 256)"
        if min(c['layers']) < 1:
            return False, f"layers={c['layers']} (a stage without blocks)"
        if self.base_width < 1 or c['input_size'] < 5:
            return False, f"input_size={c['input_size']}, base_width={self.base_width}"
        if self.layer1[0].width < 4:
            return False, f'base_width={self.base_width} (a block width of {self.layer1[0].width}, below 4)'
        h = _frequency_sizes(c['input_size'])[-1]
        if h != c['input_size'] // self.base_width:
            return False, (f"input_size={c['input_size']} with base_width={self.base_width} (the frequency size behind the four stages is {h}, "
                           f"not input_size // base_width = {c['input_size'] // self.base_width})")
        if type(self.layer1[0]) is not Bottle2neck:
            return False, 'a custom block class'
        return True, ''

    def _native_cfg(self):
        from mvector import _hip
        c = self._cfg
        cfg = _hip.MvRes2NetCfg()
        cfg.input_size, cfg.m_channels, cfg.base_width, cfg.scale, cfg.embd_dim = c['input_size'], c['m_channels'], self.base_width, self.scale, self.embd_dim
        for i in range(4):
            cfg.layers[i] = c['layers'][i]
        cfg.pooling_type = _hip.POOLING_TYPES[c['pooling_type']]
        return cfg

    def forward(self, x):
        """x: (B, T, F) -> (B, embd_dim)."""
        if self._use_native(x):
            return self._native_forward(x)
        x = self.max_pool(self.relu(self.bn1(self.conv1(x.transpose(2, 1).unsqueeze(1)))))   # (B,T,F) => (B,1,F,T)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = self.pooling(x.reshape(x.shape[0], -1, x.shape[-1]))
        return self.bn3(self.linear(self.bn2(x)))
