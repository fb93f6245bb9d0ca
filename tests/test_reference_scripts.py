"""The drop-in claim, tested on the public surface: every top-level name, public method and argument name the reference defines
in the files of the embedding path exists here.  The reference side is the stored fixture tests/golden/reference_public_api.json
(oracle/make_golden.py public_api reads the reference's sources with ``ast``); this package's side is read the same way."""
import json
import os

from conftest import PKG
from helpers import GOLDEN
from oracle.make_golden import public_api as _public_api


def _reference_api():
    with open(os.path.join(GOLDEN, 'reference_public_api.json'), encoding='utf-8') as f:
        return json.load(f)


def test_public_names_and_arguments_of_the_path_exist_here():
    """every top-level name, public method and argument name the reference defines in the files of the embedding path
    exists in this package's file of the same name (extra arguments with defaults are allowed; training-only names are listed apart)"""
    api = _reference_api()
    files = ['mvector/predict.py', 'mvector/data_utils/featurizer.py', 'mvector/metric/metrics.py', 'mvector/models/ecapa_tdnn.py', 'mvector/models/tdnn.py',
             'mvector/models/pooling.py', 'mvector/models/utils.py', 'mvector/utils/utils.py', 'mvector/utils/record.py', 'mvector/data_utils/collate_fn.py']
    missing = []
    for rel in files:
        ref, ours = api[rel], _public_api(os.path.join(PKG, rel))
        assert ref, rel
        for name, args in ref.items():
            if name not in ours:
                if name.endswith('.__init__') and name.rsplit('.', 1)[0] in ours:
                    continue   # (a constructor without arguments that the class here inherits)
                missing.append(f'{rel}: {name}')
            elif args and ours[name] is not None:
                lost = [a for a in args if a not in ours[name]]
                if lost:
                    missing.append(f'{rel}: {name} lacks {lost}')
    assert not missing, missing
    # the model files define the classes users construct (the reference's internal building blocks of CAM++ / ERes2Net are laid out differently here;
    # the state_dict contract is what test_state_dict_layout_equals_reference_manifest pins)
    for rel, names in (('mvector/models/campplus.py', ['CAMPPlus']), ('mvector/models/eres2net.py', ['ERes2Net', 'ERes2NetV2']),
                       ('mvector/trainer.py', ['MVectorTrainer', 'MVectorTrainer.evaluate', 'MVectorTrainer.train', 'MVectorTrainer.export', 'MVectorTrainer.extract_features'])):
        ref, ours = api[rel], _public_api(os.path.join(PKG, rel))
        for name in names:
            assert name in ref and name in ours, (rel, name)
        for cls in [n for n in names if '.' not in n]:
            lost = [a for a in ref[f'{cls}.__init__'] if a not in ours[f'{cls}.__init__']]
            assert not lost, (rel, cls, lost)
