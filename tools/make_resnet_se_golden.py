"""Generate the golden fixtures of ResNetSE (tests/golden/manifest_<case>.json, <case>.npz) by running the REFERENCE's own module -- the
recipe of tools/make_pooling_golden.py: the reference import of oracle/make_golden.py, the seeded weights of oracle/weights.py.

Run where the reference checkout exists (oracle/make_golden.py: REF):

    python tools/make_resnet_se_golden.py

Inputs are np.random.default_rng(seed).normal(0, 1, shape).  No weights are stored: the manifest's shapes, seed and bn_gain regenerate them.
The default model takes bn_gain 0.7: at gain 1.0 the reference's maps peak at 635, too close to the S16 limit of 1023.5 for a parity fixture.
Each case also prints the largest |map value| of the reference (forward hooks on every block, conv and the stem) and its fp32-against-fp64 1 - cos.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd')]

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
TINY = dict(input_size=16, layers=[1, 1, 1, 1], num_filters=[16, 16, 32, 32], embd_dim=64)
# case -> (constructor arguments, x shape (B, T, F), seed of weights and input, bn_gain)
CASES = {
    **{f'resnetse_tiny_{p.lower()}': (dict(TINY, pooling_type=p), (3, 41, 16), 5, 1.0) for p in ('ASP', 'SAP', 'TAP', 'TSP')},
    'resnetse_tiny2': (dict(input_size=24, layers=[2, 1, 2, 1], num_filters=[16, 32, 32, 48], embd_dim=64, pooling_type='ASP'), (2, 33, 24), 7, 1.0),
    'resnetse_default': (dict(input_size=80, pooling_type='ASP'), (2, 98, 80), 0, 0.7),
}


def main():
    from oracle import weights
    from oracle.make_golden import import_reference_models
    ref_models = import_reference_models()
    torch.set_num_threads(min(16, os.cpu_count()))
    for case, (kwargs, shape, seed, gain) in CASES.items():
        model = ref_models.ResNetSE(**kwargs)
        shapes = weights.shapes_of(model.state_dict())
        sd = weights.make_state_dict(shapes, seed, gain)
        model.load_state_dict(sd, strict=True)
        model.eval()
        x = torch.from_numpy(np.random.default_rng(seed).normal(0, 1, shape).astype(np.float32))
        peak = [0.0]
        hooks = [m.register_forward_hook(lambda _m, _i, o: peak.__setitem__(0, max(peak[0], o.abs().max().item())))
                 for m in model.modules() if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.ReLU)) or type(m).__name__ == 'SEBottleneck']
        with torch.no_grad():
            emb = model(x.clone())
            for h in hooks:
                h.remove()
            emb64 = model.double()(x.double())
        assert torch.isfinite(emb).all(), case
        d = (1 - torch.nn.functional.cosine_similarity(emb.double(), emb64, dim=1)).max().item()
        with open(os.path.join(GOLDEN, f'manifest_{case}.json'), 'w') as f:
            json.dump(dict(model='ResNetSE', kwargs=kwargs, seed=seed, bn_gain=gain, shapes={k: list(v) for k, v in shapes.items()}), f, indent=0)
        np.savez_compressed(os.path.join(GOLDEN, f'{case}.npz'), x=x.numpy(), emb=emb.numpy())
        print(f'{case}: x {tuple(x.shape)} emb {tuple(emb.shape)} |emb| {emb.abs().mean():.4f}  largest |map| {peak[0]:.1f}  fp32 vs fp64 1-cos {d:.1e}  '
              f'{sum(v.numel() for k, v in sd.items() if v.is_floating_point() and "running" not in k) / 1e6:.2f} M parameters')
    print('done ->', GOLDEN)


if __name__ == '__main__':
    main()
