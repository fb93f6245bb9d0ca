"""fp64 restatement of the SAP / TAP / TSP pooling heads (the reference's mvector/models/pooling.py: SelfAttentivePooling,
TemporalAveragePooling, TemporalStatisticsPooling) and of the two model tails behind them -- the arbiter of tests/test_pooling_heads.py and
tests/test_gpu_pooling_heads.py.  numpy float64 throughout, written from the reference's formulas, not from the kernels:

    TAP  mean_t x                                     -> [B, C]
    TSP  mean_t x | var_t x   (unbiased, T - 1; NaN at T = 1, as torch.var)   -> [B, 2C]
    SAP  sum_t softmax_t(W2 . tanh(W1 . x + b1) + b2) x                        -> [B, C]

x is channel-last here, [B, T, C] (the layout of the kernels' inputs); the reference's [B, C, T] is its transpose."""
import numpy as np
import torch


def tap(x):
    return np.asarray(x, np.float64).mean(axis=1)


def tsp(x):
    x = np.asarray(x, np.float64)
    T = x.shape[1]
    mean = x.mean(axis=1)
    ss = ((x - mean[:, None, :]) ** 2).sum(axis=1)
    var = ss / (T - 1) if T > 1 else np.full_like(mean, np.nan)
    return np.concatenate([mean, var], axis=1)


def sap_from_logits(logits, x):
    """softmax over time of logits [B, T, C], weighted sum of x [B, T, C]"""
    logits = np.asarray(logits, np.float64)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    w = e / e.sum(axis=1, keepdims=True)
    return (w * np.asarray(x, np.float64)).sum(axis=1)


def sap(x, w1, b1, w2, b2):
    """x [B, T, C]; w1 [A, C], b1 [A], w2 [C, A], b2 [C] (the Conv1d weights with the kernel axis dropped)"""
    x = np.asarray(x, np.float64)
    h = np.tanh(x @ np.asarray(w1, np.float64).T + np.asarray(b1, np.float64))
    return sap_from_logits(h @ np.asarray(w2, np.float64).T + np.asarray(b2, np.float64), x)


def head(pooling_type, x, sd, prefix):
    """the head of pooling_type over x [B, T, C] with the weights of state_dict sd under prefix ('asp' | 'pooling')"""
    if pooling_type == 'TAP':
        return tap(x)
    if pooling_type == 'TSP':
        return tsp(x)
    if pooling_type == 'SAP':
        g = lambda k: sd[f'{prefix}.{k}'].double().numpy()   # noqa: E731
        return sap(x, g('linear1.weight')[..., 0], g('linear1.bias'), g('linear2.weight')[..., 0], g('linear2.bias'))
    raise ValueError(pooling_type)


def _bn(v, sd, prefix, eps=1e-5):
    g = lambda k: sd[f'{prefix}.{k}'].double().numpy()   # noqa: E731
    return (v - g('running_mean')) / np.sqrt(g('running_var') + eps) * g('weight') + g('bias')


def pooling_input(model, x):
    """the pooling input [B, T, C] of an eval-mode TDNN / EcapaTdnn (the package's torch modules, run in fp64 on a copy)"""
    import copy
    m = copy.deepcopy(model).double().eval()
    x = torch.as_tensor(x).double()
    with torch.no_grad():
        if type(m).__name__ == 'TDNN':
            h = x.transpose(2, 1)
            for i in range(1, 5):
                h = getattr(m, f'bn{i}')(torch.relu(getattr(m, f'td_layer{i}')(h)))
            h = torch.relu(m.td_layer5(h))
        else:
            h = x.transpose(1, 2)
            outs = []
            for layer in m.blocks:
                h = layer(h)
                outs.append(h)
            h = m.mfa(torch.cat(outs[1:], dim=1))
    return h.transpose(1, 2).numpy()


def embed(model, sd, x):
    """fp64 embedding of a TDNN / EcapaTdnn with a SAP / TAP / TSP head: backbone, head of this module, tail (bn5 -> linear -> bn6 |
    asp_bn -> fc)"""
    pt = model._cfg['pooling_type']
    p = pooling_input(model, x)
    if type(model).__name__ == 'TDNN':
        v = _bn(head(pt, p, sd, 'pooling'), sd, 'bn5')
        v = v @ sd['linear.weight'].double().numpy().T + sd['linear.bias'].double().numpy()
        return _bn(v, sd, 'bn6')
    v = _bn(head(pt, p, sd, 'asp'), sd, 'asp_bn')
    return v @ sd['fc.conv.weight'].double().numpy()[..., 0].T + sd['fc.conv.bias'].double().numpy()
