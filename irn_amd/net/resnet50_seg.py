"""Segmentation network trained on the pseudo-labels: the ResNet-50 trunk at output stride 16 with a DeepLab-v2 ASPP head,
host side on PyTorch-ROCm.  Not in the reference, which leaves this step to an external DeepLab.

The trunk's module attribute names (``resnet50, stage1..4, backbone``) are those of net.resnet50_cam.Net, so its state-dict
keys are the same: a CAM checkpoint or (with the ``resnet50.`` prefix) a bare ImageNet trunk loads non-strictly, leaving only
the head's keys missing.
"""
import torch
import torch.nn as nn

from . import resnet50 as _r50

N_CLASSES = 20                        # VOC; `Net(n_classes=C)` for a dataset with another class list
ASPP_DILATIONS = (6, 12, 18, 24)
OUTPUT_STRIDE = 16


class ASPP(nn.Module):
    """DeepLab-v2's classifier: four 3x3 convolutions with bias, dilations 6 / 12 / 18 / 24, summed."""

    def __init__(self, c_in, n_out):
        super().__init__()
        self.branches = nn.ModuleList([nn.Conv2d(c_in, n_out, 3, padding=d, dilation=d, bias=True) for d in ASPP_DILATIONS])
        for m in self.branches:                 # DeepLab's initialisation of a new classifier
            nn.init.normal_(m.weight, 0.0, 0.01)
            nn.init.zeros_(m.bias)

    def forward(self, x):
        out = self.branches[0](x)
        for m in self.branches[1:]:             # a fixed order of additions
            out = out + m(x)
        return out


class Net(nn.Module):
    """[B,3,H,W] -> logits [B, n_classes + 1, ceil(H/16), ceil(W/16)] (channel 0 = background): stride 16, the last stage
    dilated by 2, frozen batch norm as everywhere here."""

    def __init__(self, n_classes=N_CLASSES):
        super().__init__()
        if not 1 <= int(n_classes) <= 80:
            raise ValueError("resnet50_seg: n_classes %s outside 1..80" % (n_classes,))
        self.n_classes = int(n_classes)
        t = _r50.resnet50(strides=(2, 2, 2, 1), dilations=(1, 1, 1, 2))
        self.resnet50 = t
        self.stage1 = _r50.Stem(t.conv1, t.bn1, t.relu, t.maxpool, t.layer1)
        self.stage2 = nn.Sequential(t.layer2)
        self.stage3 = nn.Sequential(t.layer3)
        self.stage4 = nn.Sequential(t.layer4)
        self.head = ASPP(2048, self.n_classes + 1)
        self.backbone = nn.ModuleList([self.stage1, self.stage2, self.stage3, self.stage4])

    def load_state_dict(self, state_dict, *args, **kwargs):
        """A checkpoint trained for another class list is refused by name, strict or not."""
        b = state_dict.get("head.branches.0.bias") if hasattr(state_dict, "get") else None
        if b is not None and int(b.shape[0]) != self.n_classes + 1:
            raise ValueError("resnet50_seg: the checkpoint's head has %d outputs, the network was built for %d "
                             "(--num_classes + 1)" % (int(b.shape[0]), self.n_classes + 1))
        return super().load_state_dict(state_dict, *args, **kwargs)

    def forward(self, x):
        f = _r50.to_nchw(self.stage4(self.stage3(self.stage2(self.stage1(x)))))
        return self.head(f).contiguous()

    def forward_train(self, x):
        """The same function with gradients for stages 3-4 and the head only: stages 1-2 run under `no_grad` on the inference
        path, as in net.resnet50_cam.Net.forward_train."""
        with torch.no_grad():
            x = _r50.to_nchw(self.stage2(self.stage1(x)))
        return self.head(self.stage4(self.stage3(x))).contiguous()

    def trainable_parameters(self):
        """(backbone parameters, head parameters): the optimiser's two groups, the head at ten times the rate."""
        return list(self.backbone.parameters()), list(self.head.parameters())
