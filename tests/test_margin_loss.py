"""The margin-softmax losses without a GPU: the kernels of csrc/marginloss.hip on the emulator build against the fp64 oracle of
tests/margin_loss_checks.py (tests/test_gpu_margin_loss.py runs the same checks on the device), and the host layers: the seven classes of
mvector.loss on CPU tensors against the reference's own results (tests/golden/margin_loss.npz, tools/make_margin_loss_golden.py),
SpeakerIdentification, build_loss and update()."""
import os

import numpy as np
import pytest
import torch

import margin_loss_checks as mlc
from helpers import GOLDEN


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.emu_cdll()


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'margin_loss.npz'))


@pytest.mark.parametrize('name', sorted(mlc.KINDS))
def test_emu_forward_and_backward_against_the_fp64_oracle(emu, name):
    mlc.check_kind(emu, 'cpu', name)


def test_emu_half_inputs_are_the_fp32_path_on_the_upcast_logits(emu):
    mlc.check_half_inputs(emu, 'cpu')


def test_emu_in_place_backward(emu):
    mlc.check_in_place(emu, 'cpu')


def test_emu_no_hidden_state(emu):
    mlc.check_no_hidden_state(emu, 'cpu')


def test_emu_labels_out_of_range(emu):
    mlc.check_bad_labels(emu, 'cpu')


def test_emu_nan_logit(emu):
    mlc.check_nan_logit(emu, 'cpu')


def test_emu_refusals_by_name(emu):
    mlc.check_refusals(emu, 'cpu')


def test_the_library_exports_the_margin_losses(emu):
    import ctypes
    import __graft_entry__
    from mvector import _hip
    cdll = ctypes.CDLL(__graft_entry__.build())
    header = open(os.path.join(os.path.dirname(os.path.abspath(__graft_entry__.__file__)), 'include', 'mvector_hip.h')).read()
    for name in ('mv_margin_ce_workspace_bytes', 'mv_margin_ce_forward', 'mv_margin_ce_backward'):
        assert hasattr(cdll, name) and hasattr(emu, name) and name in _hip.EXPORTED_SYMBOLS and name + '(' in header, name
    for macro in ('MV_LOSS_CE', 'MV_LOSS_AM', 'MV_LOSS_ARM', 'MV_LOSS_AAM', 'MV_LOSS_SUBCENTER', 'MV_DT_BF16', 'MV_MARGIN_SEG', 'MV_MARGIN_CHUNK',
                  'MV_MARGIN_SAVED'):
        assert f'#define {macro} {getattr(_hip, macro)}\n' in header, macro
    cdll.mv_abi_version.restype = ctypes.c_int
    assert cdll.mv_abi_version() == 5


# ------------------------------------------------------------------ host layers
def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))


def _softmax_module(name, args):
    from mvector import loss as L
    margin, scale, easy, K, eps = args
    if name == 'ce':
        return L.CELoss(label_smoothing=eps)
    if name in ('am', 'arm'):
        return {'am': L.AMLoss, 'arm': L.ARMLoss}[name](margin=margin, scale=scale, label_smoothing=eps)
    if name.startswith('aam'):
        return L.AAMLoss(margin=margin, scale=scale, easy_margin=bool(easy), label_smoothing=eps)
    return L.SubCenterLoss(margin=margin, scale=scale, easy_margin=bool(easy), K=int(K), label_smoothing=eps)


def _run_cpu(module, logits, labels, features, feature_grad=False):
    x = torch.from_numpy(logits).double().requires_grad_(True)
    f = torch.from_numpy(features).double().requires_grad_(feature_grad)
    loss = module.double()({'features': f, 'logits': x}, torch.from_numpy(labels))
    loss.backward()
    return loss.detach().numpy(), x.grad.numpy(), f.grad.numpy() if feature_grad else None


def test_cpu_path_of_all_seven_classes_meets_the_reference(golden):
    from mvector import loss as L
    labels, features = golden['labels'], golden['features']
    cases = sorted(k[:-5] for k in golden.files if k.endswith('.loss'))
    assert len(cases) == 7 * 2 + 2 + 2
    for case in cases:
        args = golden[case + '.args']
        if case.startswith('sphereface2'):
            module = L.SphereFace2(margin=args[0], scale=args[1], lanbuda=args[2], t=int(args[3]), margin_type='CA'[int(args[4])])
            with torch.no_grad():
                module.bias.fill_(-0.5)
            loss, grad, _ = _run_cpu(module, golden['logits'], labels, features)
            assert _close(module.bias.grad.numpy(), golden[case + '.bias_grad']), case
        elif case.startswith('triplet'):
            module = L.TripletAngularMarginLoss(margin=args[0], absolute_loss_weight=args[1], ap_value=args[2], an_value=args[3],
                                                label_smoothing=args[4])
            loss, grad, gfeat = _run_cpu(module, golden['logits'], labels, features, feature_grad=True)
            assert _close(gfeat, golden[case + '.grad_features']), case
        else:
            module = _softmax_module(case.rsplit('_ls', 1)[0], args)
            assert module.pred is None
            loss, grad, _ = _run_cpu(module, golden['logits_k3' if args[3] == 3 else 'logits'], labels, features)
        assert _close(loss, golden[case + '.loss']), (case, loss, golden[case + '.loss'])
        assert _close(grad, golden[case + '.grad']), case


def test_the_golden_file_covers_what_it_is_there_for(golden):
    """the branch row, |c_y| <= 1 - 2^-12, only arrays, a few tens of KB"""
    assert os.path.getsize(os.path.join(GOLDEN, 'margin_loss.npz')) < 100 * 1024
    labels = golden['labels']
    for key, k in (('logits', 1), ('logits_k3', 3)):
        c = golden[key]
        assert c.dtype == np.float32
        cy = c.reshape(len(labels), -1, k).max(axis=2)[np.arange(len(labels)), labels]
        assert np.all(np.abs(cy) <= 1 - 2.0 ** -12)
        assert cy[0] < np.cos(np.pi - 0.25) and np.all(cy[1:] > np.cos(np.pi - 0.25))
    assert all(golden[k].dtype.kind in 'fi' for k in golden.files)


def test_speaker_identification_to_loss_to_backward_on_the_cpu():
    from mvector.loss import AAMLoss, SubCenterLoss, CELoss
    from mvector.models.fc import SpeakerIdentification
    torch.manual_seed(0)
    feats = torch.randn(6, 24, requires_grad=True)
    labels = torch.tensor([0, 4, 9, 4, 1, 0])
    for head_args, loss in ((dict(), AAMLoss()), (dict(K=3), SubCenterLoss(K=3)), (dict(classifier_type='Linear'), CELoss()),
                            (dict(num_blocks=2, inter_dim=16), AAMLoss(label_smoothing=0.1))):
        head = SpeakerIdentification(24, 10, **head_args)
        out = head(feats)
        assert out['features'] is feats and out['logits'].shape == (6, 10 * head_args.get('K', 1))
        value = loss(out, labels)
        feats.grad = None
        value.backward()
        weight = head.weight if head.classifier_type == 'Cosine' else head.output.weight
        assert torch.isfinite(value) and weight.grad is not None and weight.grad.abs().sum() > 0 and feats.grad.abs().sum() > 0
    names = set(SpeakerIdentification(24, 10, num_blocks=1, inter_dim=16).state_dict())
    assert names == {'weight', 'blocks.0.linear.weight', 'blocks.0.nonlinear.batchnorm.weight', 'blocks.0.nonlinear.batchnorm.bias',
                     'blocks.0.nonlinear.batchnorm.running_mean', 'blocks.0.nonlinear.batchnorm.running_var',
                     'blocks.0.nonlinear.batchnorm.num_batches_tracked'}
    assert set(SpeakerIdentification(24, 10, classifier_type='Linear').state_dict()) == {'output.weight', 'output.bias'}
    with pytest.raises(ValueError):
        SpeakerIdentification(24, 10, classifier_type='Other')


def test_build_loss_builds_every_name_and_update_changes_the_next_result():
    from mvector import loss as L
    from mvector.utils.utils import dict_to_object
    for name in ('AAMLoss', 'AMLoss', 'ARMLoss', 'CELoss', 'SubCenterLoss', 'SphereFace2', 'TripletAngularMarginLoss'):
        args = {} if name in ('CELoss', 'TripletAngularMarginLoss') else {'margin': 0.25}
        built = L.build_loss(dict_to_object({'loss_conf': {'loss': name, 'loss_args': args}}))
        assert type(built) is getattr(L, name) and isinstance(built, torch.nn.Module)
    assert type(L.build_loss(dict_to_object({'loss_conf': {}}))) is L.AAMLoss
    with pytest.raises(AttributeError, match='FocalLoss'):
        L.build_loss(dict_to_object({'loss_conf': {'loss': 'FocalLoss'}}))
    torch.manual_seed(1)
    inputs = {'features': torch.nn.functional.normalize(torch.randn(4, 8)), 'logits': torch.rand(4, 12) * 1.8 - 0.9}
    labels = torch.tensor([0, 0, 3, 3])   # four classes where K = 3
    for module in (L.AAMLoss(), L.AMLoss(), L.ARMLoss(), L.SubCenterLoss(K=3), L.SphereFace2(), L.TripletAngularMarginLoss()):
        before = module(inputs, labels)
        module.update(margin=0.45)
        assert not torch.equal(module(inputs, labels), before), type(module).__name__
    ce = L.CELoss()
    before = ce(inputs, labels)
    ce.update(margin=0.45)
    assert torch.equal(ce(inputs, labels), before)
