"""Generate tests/golden/margin_loss.npz by running the REFERENCE's own seven loss modules (mvector/loss/*.py of the reference checkout,
loaded by path) in fp64 on seeded cosine matrices.

Run where the reference checkout exists (oracle/make_golden.py: REF):

    python tools/make_margin_loss_golden.py

Only data is written.  Shared: `features` (fp32 [B, D]), `labels` (int64 [B]), `logits` (fp32 [B, N]), `logits_k3` (fp32 [B, N * 3]).  Per case
<name>: <name>.args (fp64: the constructor arguments, see CASES), <name>.loss (fp64 scalar), <name>.grad (fp64, the gradient of the loss with
respect to the fp64 upcast of the logits); SphereFace2 cases also <name>.bias_grad, the triplet cases <name>.grad_features.

Logits: cosines of L2-normalised seeded vectors, formed in fp32 -- so every value is fp32-representable -- and handed to the reference upcast
to fp64.  Row 0's class weight is set against its feature, so its target cosine lies below th = cos(pi - margin): the `c - mmm` branch of the
angular margin.  The tool asserts |c_y| <= 1 - 2^-12 for every row (the derivative of the angular margin has 1 / sine in it) and that the
branch row is where it is meant to be.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd')]
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
B, N, D = 6, 40, 16
LABELS = [3, 3, 17, 17, 39, 39]   # pairs: the triplet loss of the reference needs the same number of positives in every row

# name: (reference module, class, constructor arguments in the order stored in <name>.args); `K` picks logits_k3
SOFTMAX = {'ce': ('celoss', 'CELoss', {}),
           'am': ('amloss', 'AMLoss', dict(margin=0.3, scale=30.0)),
           'arm': ('armloss', 'ARMLoss', dict(margin=0.3, scale=30.0)),
           'aam': ('aamloss', 'AAMLoss', dict(margin=0.25, scale=30.0, easy_margin=False)),
           'aam_easy': ('aamloss', 'AAMLoss', dict(margin=0.25, scale=30.0, easy_margin=True)),
           'subcenter': ('subcenterloss', 'SubCenterLoss', dict(margin=0.25, scale=30.0, easy_margin=False, K=3)),
           'subcenter_easy': ('subcenterloss', 'SubCenterLoss', dict(margin=0.25, scale=30.0, easy_margin=True, K=3))}
ARG_ORDER = ('margin', 'scale', 'easy_margin', 'K', 'label_smoothing')


def reference_module(name):
    from oracle.make_golden import REF
    spec = importlib.util.spec_from_file_location('ref_' + name, os.path.join(REF, 'mvector', 'loss', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cosines(rng, k):
    f = rng.standard_normal((B, D)).astype(np.float32)
    w = rng.standard_normal((N * k, D)).astype(np.float32)
    for sub in range(k):   # row 0: every sub-centre of its class points away from the feature
        w[LABELS[0] * k + sub] = -f[0] + np.float32(0.1) * rng.standard_normal(D).astype(np.float32)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    return f, (f @ w.T).astype(np.float32)


def main():
    rng = np.random.default_rng(20)
    features, logits = cosines(rng, 1)
    _, logits_k3 = cosines(rng, 3)
    labels = np.array(LABELS, dtype=np.int64)
    for c, k in ((logits, 1), (logits_k3, 3)):
        cy = c.reshape(B, N, k).max(axis=2)[np.arange(B), labels]
        assert np.all(np.abs(cy) <= 1 - 2.0 ** -12), cy
        assert cy[0] < np.cos(np.pi - 0.25) and np.all(cy[1:] > np.cos(np.pi - 0.25)), cy
    out = dict(features=features, labels=labels, logits=logits, logits_k3=logits_k3)
    y = torch.from_numpy(labels)

    def run(module, x, feats=None):
        x = torch.from_numpy(x).double().requires_grad_(True)
        f = torch.from_numpy(features).double().requires_grad_(feats is not None)
        loss = module.double()({'features': f, 'logits': x}, y)
        loss.backward()
        return loss.detach().numpy(), x.grad.numpy(), f.grad.numpy() if feats is not None else None

    for name, (mod, cls, kwargs) in SOFTMAX.items():
        for eps in (0.0, 0.1):
            args = dict(kwargs, label_smoothing=eps)
            loss, grad, _ = run(getattr(reference_module(mod), cls)(**args), logits_k3 if kwargs.get('K') == 3 else logits)
            key = f'{name}_ls{int(eps * 10)}'
            full = dict(dict(margin=0.0, scale=1.0, easy_margin=False, K=1), **args)
            out[key + '.args'] = np.array([float(full[a]) for a in ARG_ORDER])
            out[key + '.loss'], out[key + '.grad'] = loss, grad
    for mtype in 'CA':   # <name>.args: margin, scale, lanbuda, t, margin_type ('C' = 0, 'A' = 1)
        module = reference_module('sphereface2').SphereFace2(margin=0.2, scale=30.0, lanbuda=0.7, t=3, margin_type=mtype)
        with torch.no_grad():
            module.bias.fill_(-0.5)
        loss, grad, _ = run(module, logits)
        key = 'sphereface2_' + mtype
        out[key + '.args'] = np.array([0.2, 30.0, 0.7, 3.0, float(mtype == 'A')])
        out[key + '.loss'], out[key + '.grad'], out[key + '.bias_grad'] = loss, grad, module.bias.grad.numpy()
    for eps in (0.0, 0.1):   # <name>.args: margin, absolute_loss_weight, ap_value, an_value, label_smoothing
        module = reference_module('tripletangularmarginloss').TripletAngularMarginLoss(margin=0.5, absolute_loss_weight=0.7, ap_value=0.8,
                                                                                       an_value=0.1, label_smoothing=eps)
        loss, grad, gfeat = run(module, logits, feats=True)
        key = f'triplet_ls{int(eps * 10)}'
        out[key + '.args'] = np.array([0.5, 0.7, 0.8, 0.1, eps])
        out[key + '.loss'], out[key + '.grad'], out[key + '.grad_features'] = loss, grad, gfeat
    path = os.path.join(GOLDEN, 'margin_loss.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
