"""Generate the golden fixtures of the SAP / TAP / TSP pooling heads (tests/golden/manifest_<case>.json, <case>.npz) by running the
REFERENCE's own TDNN and EcapaTdnn modules with `pooling_type` set -- the recipe of oracle/make_golden.py::save_eres2net_golden, which this
reuses (the reference import, the seeded weights) without touching the fixtures it writes.

Run where the reference checkout exists (oracle/make_golden.py: REF):

    python tools/make_pooling_golden.py

The inputs are those of the ASP fixtures of the same shapes (tests/golden/tdnn.npz, ecapa_tiny.npz, ecapa_c1024.npz), so a head's golden
differs from its ASP golden in the head alone.  No weights are stored: the manifest's shapes and seed regenerate them (oracle/weights.py).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'voiceprintrecognition-pytorch_amd')]

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
HEADS = ('SAP', 'TAP', 'TSP')
# case stem -> (model, constructor arguments, weight seed, ASP fixture whose input x is reused; its shape (B, T, F))
STEMS = {
    'tdnn_{}': ('TDNN', dict(input_size=80), 0, 'tdnn'),                                                    # (4, 98, 80)
    'ecapa_{}_tiny': ('EcapaTdnn', dict(input_size=80, channels=[64, 64, 64, 64, 192]), 3, 'ecapa_tiny'),   # (3, 50, 80)
    'ecapa_{}_c1024': ('EcapaTdnn', dict(input_size=80, channels=[1024, 1024, 1024, 1024, 3072]), 0, 'ecapa_c1024'),   # (2, 298, 80)
}
SHAPES = {'tdnn': (4, 98, 80), 'ecapa_tiny': (3, 50, 80), 'ecapa_c1024': (2, 298, 80)}


def cases():
    for stem, (cls, kwargs, seed, src) in STEMS.items():
        for head in HEADS:
            yield stem.format(head.lower()), cls, dict(kwargs, pooling_type=head), seed, src


def main():
    from oracle import weights
    from oracle.make_golden import import_reference_models
    ref_models = import_reference_models()
    torch.set_num_threads(min(16, os.cpu_count()))
    for case, cls, kwargs, seed, src in cases():
        model = getattr(ref_models, cls)(**kwargs)
        shapes = weights.shapes_of(model.state_dict())
        sd = weights.make_state_dict(shapes, seed)
        model.load_state_dict(sd, strict=True)
        model.eval()
        x = torch.from_numpy(np.load(os.path.join(GOLDEN, f'{src}.npz'))['x'])
        assert tuple(x.shape) == SHAPES[src], (src, x.shape)
        with torch.no_grad():
            emb = model(x.clone())
        assert torch.isfinite(emb).all(), case
        with open(os.path.join(GOLDEN, f'manifest_{case}.json'), 'w') as f:
            json.dump(dict(model=cls, kwargs=kwargs, seed=seed, input_from=src, shapes={k: list(v) for k, v in shapes.items()}), f, indent=0)
        np.savez_compressed(os.path.join(GOLDEN, f'{case}.npz'), x=x.numpy(), emb=emb.numpy())
        print(f'{case}: x {tuple(x.shape)} emb {tuple(emb.shape)} |emb| {emb.abs().mean():.4f}')
    print('done ->', GOLDEN)


if __name__ == '__main__':
    main()
