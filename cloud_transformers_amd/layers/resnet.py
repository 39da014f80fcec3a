"""ResNet-50 with torchvision's module tree and state-dict names, for the image encoder of the single-view reconstruction
model (model_zoo/image_reconstruction/reconstructor.py:16-33: `ResNet50Bottom(models.resnet50(pretrained=True))`) where
torchvision is not installed.  `conv1, bn1, relu, maxpool, layer1..4, avgpool, fc` in that order, so that the reference's
`list(model.children())[:-2]` is the convolutional trunk and its keys are `res50_model.0.features.<k>. ...`; released
checkpoints load with `strict=True`.  Torchvision's v1.5 form: the stride sits on the 3x3 convolution.  The convolutions stay on
torch (MIOpen): the encoder is plumbing around the hot path, not part of it.

`torchvision_stand_in()` is the module pair `harness.get_model` offers a model file when `import torchvision` fails."""
import os
import sys
import types
import warnings

import torch
from torch import nn

WEIGHTS_ENV = "CLOUDCT_RESNET50_WEIGHTS"
_warned = False


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


class ResNet(nn.Module):
    def __init__(self, layers, num_classes=1000):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], stride=2)
        self.layer3 = self._make_layer(256, layers[2], stride=2)
        self.layer4 = self._make_layer(512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * Bottleneck.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * Bottleneck.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * Bottleneck.expansion, kernel_size=1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * Bottleneck.expansion))
        layers = [Bottleneck(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * Bottleneck.expansion
        layers += [Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def resnet50(pretrained=False, **kwargs):
    """torchvision.models.resnet50's module tree, randomly initialised as torchvision initialises it.  `pretrained=True` loads
    the state dict of the file the environment variable CLOUDCT_RESNET50_WEIGHTS names (torchvision's resnet50 .pth,
    `strict=True`) when it is set; otherwise it warns once and keeps the random initialisation — nothing is ever downloaded, and
    a restored checkpoint overwrites the encoder anyway."""
    global _warned
    model = ResNet([3, 4, 6, 3], **kwargs)
    if pretrained:
        path = os.environ.get(WEIGHTS_ENV)
        if path:
            model.load_state_dict(torch.load(path, map_location="cpu"), strict=True)
        elif not _warned:
            _warned = True
            warnings.warn("resnet50(pretrained=True): torchvision is not installed and %s is not set; the encoder keeps its random "
                          "initialisation (a restored checkpoint overwrites it)" % WEIGHTS_ENV)
    return model


def torchvision_stand_in():
    """{"torchvision": module, "torchvision.models": module}: the small pair that lets `import torchvision.models as models;
    models.resnet50(...)` of a model file work without torchvision."""
    tv, models = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
    models.resnet50 = resnet50
    tv.models = models
    tv.__doc__ = models.__doc__ = "stand-in of cloud_transformers_amd.layers.resnet: offers resnet50 only"
    return {"torchvision": tv, "torchvision.models": models}


class stand_in_for_torchvision(object):
    """Context: when `import torchvision` fails, the stand-in pair sits in sys.modules inside the block and is removed
    afterwards; when torchvision is importable, nothing changes."""

    def __enter__(self):
        self.added = []
        try:
            import torchvision  # noqa: F401
        except ImportError:
            for name, mod in torchvision_stand_in().items():
                if name not in sys.modules:
                    sys.modules[name] = mod
                    self.added.append(name)
        return self

    def __exit__(self, *exc):
        for name in self.added:
            sys.modules.pop(name, None)
        return False
