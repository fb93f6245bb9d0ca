"""Generate the golden fixtures of Res2Net (tests/golden/manifest_<case>.json, <case>.npz) by running the REFERENCE's own module -- the
recipe of tools/make_resnet_se_golden.py: the reference import of oracle/make_golden.py, the seeded weights of oracle/weights.py.

Run where the reference checkout exists (oracle/make_golden.py: REF):

    python tools/make_res2net_golden.py

Inputs are np.random.default_rng(seed).normal(0, 1, shape).  No weights are stored: the manifest's shapes, seed and bn_gain regenerate them.
The default model takes bn_gain 0.7: at gain 1.0 the reference's maps peak at 12 378, far beyond the S16 limit of 1023.5.
Each case also prints the largest |map value| of the reference (forward hooks on the stem, the pools, every conv + BatchNorm and every block) and
its fp32-against-fp64 1 - cos.  A parity fixture has to stay below 512, half the S16 range: asserted.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd')]

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
TINY = dict(input_size=32, m_channels=16, layers=[1, 1, 1, 1], base_width=32, scale=2, embd_dim=64)   # widths 8 / 16 / 32 / 64: ragged slices
# case -> (constructor arguments, x shape (B, T, F), seed of weights and input, bn_gain)
CASES = {
    **{f'res2net_tiny_{p.lower()}': (dict(TINY, pooling_type=p), (3, 101, 32), 5, 1.0) for p in ('ASP', 'SAP', 'TAP', 'TSP')},
    # widths 4 / 8 / 16 / 32, three 3x3 convs per block, 'normal' blocks with the sp + spx[i] chain
    'res2net_tiny_s4': (dict(input_size=16, m_channels=16, layers=[2, 1, 2, 1], base_width=16, scale=4, embd_dim=64, pooling_type='ASP'), (2, 53, 16), 7, 1.0),
    # scale 1: no last slice, the one conv sees everything
    'res2net_tiny_s1': (dict(input_size=32, m_channels=16, layers=[1, 2, 1, 1], base_width=32, scale=1, embd_dim=64, pooling_type='TSP'), (2, 70, 32), 9, 1.0),
    'res2net_default': (dict(input_size=80, pooling_type='ASP'), (2, 98, 80), 0, 0.7),
}
PEAK_LIMIT = 512.0


def main():
    from oracle import weights
    from oracle.make_golden import import_reference_models
    ref_models = import_reference_models()
    torch.set_num_threads(min(16, os.cpu_count()))
    for case, (kwargs, shape, seed, gain) in CASES.items():
        model = ref_models.Res2Net(**kwargs)
        shapes = weights.shapes_of(model.state_dict())
        sd = weights.make_state_dict(shapes, seed, gain)
        model.load_state_dict(sd, strict=True)
        model.eval()
        x = torch.from_numpy(np.random.default_rng(seed).normal(0, 1, shape).astype(np.float32))
        peak = [0.0]
        kinds = (torch.nn.BatchNorm2d, torch.nn.ReLU, torch.nn.MaxPool2d, torch.nn.AvgPool2d)
        hooks = [m.register_forward_hook(lambda _m, _i, o: peak.__setitem__(0, max(peak[0], o.abs().max().item())))
                 for m in model.modules() if isinstance(m, kinds) or type(m).__name__ == 'Bottle2neck']
        with torch.no_grad():
            emb = model(x.clone())
            for h in hooks:
                h.remove()
            emb64 = model.double()(x.double())
        assert torch.isfinite(emb).all(), case
        assert peak[0] < PEAK_LIMIT, (case, peak[0])
        d = (1 - torch.nn.functional.cosine_similarity(emb.double(), emb64, dim=1)).max().item()
        with open(os.path.join(GOLDEN, f'manifest_{case}.json'), 'w') as f:
            json.dump(dict(model='Res2Net', kwargs=kwargs, seed=seed, bn_gain=gain, shapes={k: list(v) for k, v in shapes.items()}), f, indent=0)
        np.savez_compressed(os.path.join(GOLDEN, f'{case}.npz'), x=x.numpy(), emb=emb.numpy())
        print(f'{case}: x {tuple(x.shape)} emb {tuple(emb.shape)} |emb| {emb.abs().mean():.4f}  largest |map| {peak[0]:.1f}  fp32 vs fp64 1-cos {d:.1e}  '
              f'{sum(v.numel() for k, v in sd.items() if v.is_floating_point() and "running" not in k) / 1e6:.2f} M parameters')
    print('done ->', GOLDEN)


if __name__ == '__main__':
    main()
