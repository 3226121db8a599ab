"""A plain-torch.nn restatement of the SSCD network (`sscd_disc_mixup.torchscript.pt`), written from its public description -- neither
the file nor torchvision was available: a torchvision-layout ResNet-50 (Bottleneck blocks [3, 4, 6, 3], the stride on the 3 x 3
conv2, BatchNorm eps 1e-5) under the prefix `backbone.`, its average pool replaced by GeM pooling
`x.clamp(min=1e-6).pow(p).mean((2, 3)).pow(1 / p)` with p = 3, its fc a 2048 -> 512 linear layer, then `F.normalize(x, dim=1)`.
23,508,032 trunk + 1,049,088 linear = 24,557,120 parameters.  Scriptable (torch.jit.script), runs in f32 or f64; `make(seed)` also
randomises every BatchNorm's weight, bias and running statistics so that folding them is exercised.  The controls of
tests/test_hip_sscd.py are switches of this module: the stride on conv1 instead of conv2, average pooling instead of GeM, and
the BN statistics reset."""
import torch
import torch.nn as nn
import torch.nn.functional as F

PARAMETERS = 24_557_120
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class Bottleneck(nn.Module):
    def __init__(self, inplanes: int, width: int, stride: int, downsample: bool, stride_on_conv1: bool = False):
        super().__init__()
        s1, s2 = (stride, 1) if stride_on_conv1 else (1, stride)
        self.conv1 = nn.Conv2d(inplanes, width, 1, s1, 0, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, s2, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, 4 * width, 1, 1, 0, bias=False)
        self.bn3 = nn.BatchNorm2d(4 * width)
        self.relu = nn.ReLU()
        self.downsample = None
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, 4 * width, 1, stride, 0, bias=False), nn.BatchNorm2d(4 * width))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(out + x)


class Backbone(nn.Module):
    def __init__(self, dims: int, pool_param: float, stride_on_conv1: bool, gem: bool):
        super().__init__()
        self.p, self.gem = pool_param, gem
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU()
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inp = 64
        layers = []
        for i, (width, n) in enumerate(zip((64, 128, 256, 512), (3, 4, 6, 3))):
            blocks = []
            for j in range(n):
                blocks.append(Bottleneck(inp, width, 2 if (i > 0 and j == 0) else 1, j == 0, stride_on_conv1))
                inp = 4 * width
            layers.append(nn.Sequential(*blocks))
        self.layer1, self.layer2, self.layer3, self.layer4 = layers
        self.fc = nn.Linear(2048, dims)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        if self.gem:
            x = x.clamp(min=1e-6).pow(self.p).mean((2, 3)).pow(1.0 / self.p)
        else:
            x = x.mean((2, 3))
        return self.fc(x)


class SSCD(nn.Module):
    def __init__(self, dims: int = 512, pool_param: float = 3.0, stride_on_conv1: bool = False, gem: bool = True):
        super().__init__()
        self.backbone = Backbone(dims, pool_param, stride_on_conv1, gem)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return F.normalize(self.backbone(x), dim=1)


def randomise_bn(net, generator):
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            n = m.num_features
            m.weight.data = 0.75 + 0.5 * torch.rand(n, generator=generator)
            m.bias.data = 0.2 * torch.randn(n, generator=generator)
            m.running_mean.data = 0.2 * torch.randn(n, generator=generator)
            m.running_var.data = 0.5 + torch.rand(n, generator=generator)
    return net


def make(seed, **kw):
    """A random-init network in eval mode under `seed`: torchvision's initialisation (convolutions kaiming-normal over fan_out, so
    that the image still matters at layer4; nn.Linear's default for fc), every BatchNorm randomised."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = SSCD(**kw)
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    return randomise_bn(net, torch.Generator().manual_seed(seed + 1)).eval()


def variant(net, **kw):
    """The same weights in a network built with other switches (a negative control)."""
    other = SSCD(**kw)
    other.load_state_dict(net.state_dict())
    return other.eval()


def reset_bn(net):
    """A copy with every BatchNorm's running statistics reset to 0 / 1 (a negative control)."""
    other = variant(net)
    for m in other.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.reset_running_stats()
    return other


@torch.no_grad()
def embed(net, x, dtype=torch.float64, device="cpu"):
    """The embeddings of normalised images x [N, 3, H, W] with the network and the images in `dtype` on `device`, returned as f64
    on the host (`net` itself is left as it is)."""
    import copy
    m = copy.deepcopy(net).to(device=device, dtype=dtype).eval()
    return m(x.to(device=device, dtype=dtype)).double().cpu()


def normalise(u8, mean, std):
    """Normalize(mean, std)(ToTensor(.)) of uint8 images [n, H, W, 3] in f32, as torch computes it on the host."""
    x = u8.permute(0, 3, 1, 2).float().div(255)
    m = torch.tensor(mean, dtype=torch.float32).view(-1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(-1, 1, 1)
    return (x - m) / s
