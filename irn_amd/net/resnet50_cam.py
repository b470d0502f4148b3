"""CAM classifier backbone (inference form, and the classifier's training forward), host side on PyTorch-ROCm.

API mirror of reference net/resnet50_cam.py: module attribute names (``resnet50, stage1..4,
classifier, backbone, newly_added``) reproduce the reference's state-dict keys, aliases included,
so ``load_state_dict(torch.load('res50_cam.pth'), strict=True)`` (step/make_cam.py:64) works.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import resnet50 as _r50

N_CLASSES = 20                        # VOC; `Net(n_classes=C)` for a dataset with another class list


class Net(nn.Module):
    """Classifier form (net/resnet50_cam.py:7-47): its parameters are what the label steps load; `forward_train` and
    `trainable_parameters` are what step/train_cam.py trains them with."""

    def __init__(self, n_classes=N_CLASSES):
        super().__init__()
        if not 1 <= int(n_classes) <= 80:
            raise ValueError("resnet50_cam: n_classes %s outside 1..80" % (n_classes,))
        self.n_classes = int(n_classes)
        t = _r50.resnet50(strides=(2, 2, 2, 1))
        self.resnet50 = t
        self.stage1 = _r50.Stem(t.conv1, t.bn1, t.relu, t.maxpool, t.layer1)
        self.stage2 = nn.Sequential(t.layer2)
        self.stage3 = nn.Sequential(t.layer3)
        self.stage4 = nn.Sequential(t.layer4)
        self.classifier = nn.Conv2d(2048, self.n_classes, 1, bias=False)
        self.backbone = nn.ModuleList([self.stage1, self.stage2, self.stage3, self.stage4])
        self.newly_added = nn.ModuleList([self.classifier])

    def load_state_dict(self, state_dict, *args, **kwargs):
        """A checkpoint trained for another class list is refused by name (strict or not: a classifier of another width can
        be neither loaded nor skipped)."""
        w = state_dict.get("classifier.weight") if hasattr(state_dict, "get") else None
        if w is not None and int(w.shape[0]) != self.n_classes:
            raise ValueError("resnet50_cam: the checkpoint's classifier has %d classes, the network was built for %d "
                             "(--num_classes)" % (int(w.shape[0]), self.n_classes))
        return super().load_state_dict(state_dict, *args, **kwargs)

    def features(self, x):
        return self.stage4(self.stage3(self.stage2(self.stage1(x))))

    def forward(self, x):
        f = self.features(x)
        _r50.end_trunk_pass()
        return self.classifier(f.mean(dim=(2, 3), keepdim=True)).flatten(1)


    def forward_train(self, x):
        """[B,3,H,W] -> logits [B,n_classes] with gradients for stages 3-4 and the classifier only (net/resnet50_cam.py:25-37).
        The reference detaches stage 2's output and no parameter of stages 1-2 ever receives a gradient; here that half
        runs under `no_grad` instead — the same function and the same gradients, but no activation of it is saved and it
        takes the inference path (fused batch norm passes).  Stages 3-4 are composed PyTorch ops under autograd, or with
        `resnet50.TRAIN_FUSED_TAIL` the differentiable fused tail (`ops.bn_act`)."""
        with torch.no_grad():
            x = _r50.to_nchw(self.stage2(self.stage1(x)))
        f = self.stage4(self.stage3(x))
        return self.classifier(f.mean(dim=(2, 3), keepdim=True)).flatten(1)

    def trainable_parameters(self):
        """(backbone parameters, newly added parameters): the optimiser's two groups (net/resnet50_cam.py:45-47)."""
        return list(self.backbone.parameters()), list(self.newly_added.parameters())


class CAM(Net):
    """[2,3,H,W] (image, h-flipped image) -> [n_classes, ceil(H/16), ceil(W/16)] activation maps:
    relu(1x1 conv with the classifier weights), original + flipped-back (net/resnet50_cam.py:55-70)."""

    def forward(self, x):
        a = _r50.to_nchw(F.relu(F.conv2d(self.features(x), self.classifier.weight)))
        return a[0] + a[1].flip(-1)

    def forward_batch(self, x):
        """[2B,3,H,W] = B (image, h-flipped image) pairs of ONE size back to back -> [B,n_classes,h,w]: the forward above for
        every pair in one pass of the trunk (the steps stack the images of a size group per scale).  In the reproducible
        mode the rows travel in passes of a fixed size per image size (`resnet50.run_rows`): a pair's maps do not depend on
        what else is in `x`."""
        a = _r50.run_rows(self._maps, x)
        return a[0::2] + a[1::2].flip(-1)

    def _maps(self, x):
        return _r50.to_nchw(F.relu(F.conv2d(self.features(x), self.classifier.weight)))
