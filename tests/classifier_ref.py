"""CPU restatement of the MNIST ResNet-18 of the quality metrics (test infrastructure only), written from its architecture:

    conv1 7x7/2 pad 3 (Cin 1 or 3 -> 64, no bias) -> BN -> ReLU -> maxpool 3x3/2 pad 1
    layer1..4: two BasicBlocks each, widths 64 / 128 / 256 / 512; the first block of layers 2-4 has stride 2 and a
               1x1/2 conv + BN shortcut.  BasicBlock: conv3x3 -> BN -> ReLU -> conv3x3 -> BN, + shortcut, ReLU
    no avgpool: fc (512 -> num_classes) on the flattened 512 x 1 x 1 map

State-dict key names are torch's for that module tree (conv1, bn1, layer{i}.{j}.{conv1,bn1,conv2,bn2}, layer{i}.0.downsample.{0,1}, fc).
Run it in eval mode; `.double()` gives the f64 reference the HIP logits are held against."""
import copy
import math

import torch
from torch import nn


class Block(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        h = torch.relu(self.bn1(self.conv1(x)))
        h = self.bn2(self.conv2(h))
        return torch.relu(h + (x if self.downsample is None else self.downsample(x)))


class ResNet18Ref(nn.Module):
    def __init__(self, num_classes=10, grayscale=True):
        super().__init__()
        self.conv1 = nn.Conv2d(1 if grayscale else 3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cin = 64
        for i, w in enumerate((64, 128, 256, 512), 1):
            s = 1 if i == 1 else 2
            setattr(self, f"layer{i}", nn.Sequential(Block(cin, w, s), Block(w, w, 1)))
            cin = w
        self.fc = nn.Linear(512, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                k = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2.0 / k))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def forward(self, x):
        x = self.maxpool(torch.relu(self.bn1(self.conv1(x))))
        for i in range(1, 5):
            x = getattr(self, f"layer{i}")(x)
        return self.fc(x.flatten(1))


def make(num_classes=10, grayscale=True, seed=0, randomize_bn=True):
    """A reference-initialised network (seeded), in eval mode; randomize_bn: gamma in [0.5, 1.5], beta and mean in [-0.2, 0.2],
    var in [0.5, 2] so that the folded BN is exercised."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = ResNet18Ref(num_classes, grayscale)
    if randomize_bn:
        g = torch.Generator().manual_seed(seed + 1)
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.weight.data = torch.rand(c, generator=g) + 0.5
                m.bias.data = torch.rand(c, generator=g) * 0.4 - 0.2
                m.running_mean.data = torch.rand(c, generator=g) * 0.4 - 0.2
                m.running_var.data = torch.rand(c, generator=g) * 1.5 + 0.5
    return net.eval()


def reset_bn_stats(sd):
    """The same state dict with the BN running statistics back at 0 / 1 (the negative control)."""
    out = {k: v.clone() for k, v in sd.items()}
    for k in out:
        if k.endswith("running_mean"):
            out[k].zero_()
        elif k.endswith("running_var"):
            out[k].fill_(1)
    return out


@torch.no_grad()
def logits_f64(net, x):
    return copy.deepcopy(net).double()(x.double())


def inception_score_f64(logits, splits, perm, remove_class=None):
    """f64 restatement of the score: drop rows / column of remove_class (splits - 1 splits), permute by `perm`, per torch.chunk
    split exp(mean_i KL(p_i || mean p)), then (mean, unbiased std) over the splits."""
    lg = logits.double()
    if remove_class is not None:
        lg = lg[lg.argmax(-1) != remove_class]
        lg = lg[:, [c for c in range(lg.shape[1]) if c != remove_class]]
        splits = splits - 1
    lg = lg[perm]
    n = lg.shape[0]
    size = -(-n // splits)                      # torch.chunk: chunks of ceil(n / splits) rows, the last one shorter
    scores = []
    for s in range(0, n, size):
        c = lg[s:s + size]
        p = torch.softmax(c, dim=1)
        lp = torch.log_softmax(c, dim=1)
        mp = p.mean(dim=0, keepdim=True)
        scores.append(math.exp(float((p * (lp - mp.log())).sum(dim=1).mean())))
    k = len(scores)
    mean = sum(scores) / k
    std = math.sqrt(sum((v - mean) ** 2 for v in scores) / (k - 1)) if k > 1 else float("nan")
    return mean, std, k
