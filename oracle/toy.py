"""Small deterministic stand-in network used for fixtures (oracle; test infrastructure only).

Float32 parameters and outputs, float64 arithmetic inside: torch's float32 CPU kernels (randn, tanh, convolution
reductions) round differently with the CPU's vector ISA and the thread count, so a float32 network would make the golden
vectors a record of one machine.  Rounded once from float64, the weights and every output are the same on any host."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class ToyEps(nn.Module):
    """Deterministic stand-in for ``unet`` (time-conditioned 2-conv net, ~2k params)."""

    def __init__(self, c, hidden=8, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.c1 = nn.Conv2d(c, hidden, 3, padding=1)
        self.c2 = nn.Conv2d(hidden, c, 3, padding=1)
        self.te = nn.Linear(1, hidden)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_((torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.2).float())

    def forward(self, x, t, return_dict=False, **kw):
        d = lambda p: p.double()
        te = F.linear(t.double()[:, None] / 1000.0, d(self.te.weight), d(self.te.bias))
        h = F.conv2d(x.double(), d(self.c1.weight), d(self.c1.bias), padding=1) + te[:, :, None, None]
        return (F.conv2d(torch.tanh(h), d(self.c2.weight), d(self.c2.bias), padding=1).to(x.dtype),)
