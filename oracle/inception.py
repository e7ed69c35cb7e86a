"""TEST INFRASTRUCTURE (oracle): torch-CPU fp32 restatement of the FID InceptionV3 forward — torchvision's published Inception3
architecture with the reference's FID patches (reference pytorch_fid/inception.py:129-163 forward, :193-310 patched blocks;
torchvision.models.inception: BasicConv2d = conv(bias=False) + BatchNorm2d(eps=1e-3) + ReLU, InceptionA / B / C / D / E).

PARITY UNPINNED: torchvision and the FID weight file (pt_inception-2015-12-05-6726825d.pth) are absent from this image, so nothing
the reference itself computes can be reproduced here; this restatement follows the published layer tables and is what the HIP
program (diffusion-by-maxentirl_amd/pytorch_fid/inception.py) is checked against, on formula weights.  Functional over a state
dict with torchvision's names.  Only tests/ may import this module."""
import torch
import torch.nn.functional as F


class Graph:
    """The operations the architecture below is wired from.  This default is the torch-CPU fp32 oracle; a caller may pass a
    subclass to forward() / the inception_* functions to walk the same wiring over other values (tests/inception_walk.py walks it
    over the device tensors of the HIP run).  `where` names the call site of a pool: "<block>.pool" inside a Mixed block,
    "pool1" / "pool2" after the two stem blocks, "pool3" for the global average."""

    def prep(self, x, resize_input, normalize_input):
        if resize_input:
            x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
        if normalize_input:
            x = 2 * x - 1
        return x

    def bc(self, sd, name, x, stride=1, padding=0):
        """BasicConv2d in eval mode."""
        x = F.conv2d(x, sd[name + ".conv.weight"], None, stride=stride, padding=padding)
        x = F.batch_norm(x, sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"], sd[name + ".bn.weight"], sd[name + ".bn.bias"],
                         training=False, eps=1e-3)
        return F.relu(x)

    def avg(self, where, x):
        return F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)        # the FID patch

    def maxpool(self, where, x, stride, padding=0):
        return F.max_pool2d(x, kernel_size=3, stride=stride, padding=padding)

    def gap(self, where, x):
        return F.adaptive_avg_pool2d(x, (1, 1))


TORCH = Graph()


def _bc(sd, name, x, stride=1, padding=0):
    return TORCH.bc(sd, name, x, stride, padding)


def _avg(x):
    return TORCH.avg("", x)


def inception_a(sd, p, x, g=TORCH):
    b1 = g.bc(sd, p + ".branch1x1", x)
    b5 = g.bc(sd, p + ".branch5x5_2", g.bc(sd, p + ".branch5x5_1", x), padding=2)
    b3 = g.bc(sd, p + ".branch3x3dbl_3", g.bc(sd, p + ".branch3x3dbl_2", g.bc(sd, p + ".branch3x3dbl_1", x), padding=1), padding=1)
    return torch.cat([b1, b5, b3, g.bc(sd, p + ".branch_pool", g.avg(p + ".pool", x))], 1)


def inception_b(sd, p, x, g=TORCH):
    b3 = g.bc(sd, p + ".branch3x3", x, stride=2)
    bd = g.bc(sd, p + ".branch3x3dbl_3", g.bc(sd, p + ".branch3x3dbl_2", g.bc(sd, p + ".branch3x3dbl_1", x), padding=1), stride=2)
    return torch.cat([b3, bd, g.maxpool(p + ".pool", x, 2)], 1)


def inception_c(sd, p, x, g=TORCH):
    b1 = g.bc(sd, p + ".branch1x1", x)
    b7 = g.bc(sd, p + ".branch7x7_3", g.bc(sd, p + ".branch7x7_2", g.bc(sd, p + ".branch7x7_1", x), padding=(0, 3)), padding=(3, 0))
    bd = g.bc(sd, p + ".branch7x7dbl_2", g.bc(sd, p + ".branch7x7dbl_1", x), padding=(3, 0))
    bd = g.bc(sd, p + ".branch7x7dbl_4", g.bc(sd, p + ".branch7x7dbl_3", bd, padding=(0, 3)), padding=(3, 0))
    bd = g.bc(sd, p + ".branch7x7dbl_5", bd, padding=(0, 3))
    return torch.cat([b1, b7, bd, g.bc(sd, p + ".branch_pool", g.avg(p + ".pool", x))], 1)


def inception_d(sd, p, x, g=TORCH):
    b3 = g.bc(sd, p + ".branch3x3_2", g.bc(sd, p + ".branch3x3_1", x), stride=2)
    b7 = g.bc(sd, p + ".branch7x7x3_3", g.bc(sd, p + ".branch7x7x3_2", g.bc(sd, p + ".branch7x7x3_1", x), padding=(0, 3)), padding=(3, 0))
    b7 = g.bc(sd, p + ".branch7x7x3_4", b7, stride=2)
    return torch.cat([b3, b7, g.maxpool(p + ".pool", x, 2)], 1)


def inception_e(sd, p, x, max_pool, g=TORCH):
    b1 = g.bc(sd, p + ".branch1x1", x)
    t = g.bc(sd, p + ".branch3x3_1", x)
    b3 = torch.cat([g.bc(sd, p + ".branch3x3_2a", t, padding=(0, 1)), g.bc(sd, p + ".branch3x3_2b", t, padding=(1, 0))], 1)
    t = g.bc(sd, p + ".branch3x3dbl_2", g.bc(sd, p + ".branch3x3dbl_1", x), padding=1)
    bd = torch.cat([g.bc(sd, p + ".branch3x3dbl_3a", t, padding=(0, 1)), g.bc(sd, p + ".branch3x3dbl_3b", t, padding=(1, 0))], 1)
    pooled = g.maxpool(p + ".pool", x, 1, 1) if max_pool else g.avg(p + ".pool", x)      # Mixed_7c's max pool: inception.py:303-308
    return torch.cat([b1, b3, bd, g.bc(sd, p + ".branch_pool", pooled)], 1)


def forward(sd, inp, resize_input=True, normalize_input=True, last_block=3, g=TORCH):
    """-> list of the four blocks' outputs (reference InceptionV3.forward with output_blocks = 0..last_block)."""
    x = g.prep(inp, resize_input, normalize_input)
    outs = []
    x = g.bc(sd, "Conv2d_2b_3x3", g.bc(sd, "Conv2d_2a_3x3", g.bc(sd, "Conv2d_1a_3x3", x, stride=2)), padding=1)
    x = g.maxpool("pool1", x, 2)
    outs.append(x)
    if last_block >= 1:
        x = g.maxpool("pool2", g.bc(sd, "Conv2d_4a_3x3", g.bc(sd, "Conv2d_3b_1x1", x)), 2)
        outs.append(x)
    if last_block >= 2:
        for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            x = inception_a(sd, n, x, g)
        x = inception_b(sd, "Mixed_6a", x, g)
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = inception_c(sd, n, x, g)
        outs.append(x)
    if last_block >= 3:
        x = inception_d(sd, "Mixed_7a", x, g)
        x = inception_e(sd, "Mixed_7b", x, False, g)
        x = inception_e(sd, "Mixed_7c", x, True, g)
        outs.append(g.gap("pool3", x))
    return outs
