"""Classification losses of the training recipes: ``build_loss(configs)`` builds the class named by ``configs.loss_conf.loss`` (default
AAMLoss) with ``loss_args``, the reference's contract (mvector/loss/__init__.py).

``CELoss``, ``AMLoss``, ``ARMLoss``, ``AAMLoss`` and ``SubCenterLoss`` are one softmax family (mvector/loss/softmax_family.py): on 2-D CUDA
logits of fp32, fp16 or bf16 they run the fused native forward and backward (csrc/marginloss.hip) behind one ``torch.autograd.Function``;
on CPU tensors and every other dtype they run the same definition as a torch expression.  ``SphereFace2`` (csrc/sphereface2.hip) and
``TripletAngularMarginLoss`` (csrc/triplet.hip, its cross-entropy through the family's native function) take their native paths under the
same conditions, and run their torch expressions otherwise."""
from mvector.utils.logger import logger
from .softmax_family import AAMLoss, AMLoss, ARMLoss, CELoss, SubCenterLoss
from .sphereface2 import SphereFace2
from .triplet import TripletAngularMarginLoss

LOSSES = {cls.__name__: cls for cls in (AAMLoss, AMLoss, ARMLoss, CELoss, SphereFace2, SubCenterLoss, TripletAngularMarginLoss)}
__all__ = ['build_loss'] + sorted(LOSSES)


def build_loss(configs):
    conf = configs.loss_conf
    name = conf.get('loss', 'AAMLoss')
    if name not in LOSSES:
        raise AttributeError(f"module 'mvector.loss' has no attribute '{name}' (available: {sorted(LOSSES)})")
    kwargs = conf.get('loss_args', {})
    loss = LOSSES[name](**kwargs)
    logger.info(f'成功创建损失函数：{name}，参数为：{kwargs}')
    return loss
