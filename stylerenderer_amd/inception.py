"""The FID Inception-v3 trunk: the network of the reference's calc_inception.load_patched_inception_v3(), i.e.
inception.InceptionV3([3], normalize_input=False) on fid_inception_v3(), returning the 2048 pooled features.

    input        the generator's image in [-1, 1], unscaled; resized to 299^2 with
                 F.interpolate(mode='bilinear', align_corners=False) when it is not 299^2 (inception.py:139-143)
    stem         Conv2d_1a_3x3 (/2) -> 2a -> 2b (pad 1) -> max 3x3/2 -> 3b_1x1 -> 4a_3x3 -> max 3x3/2
    blocks       Mixed_5b/5c/5d FIDInceptionA (pool features 32/64/64), Mixed_6a InceptionB, Mixed_6b-6e FIDInceptionC
                 (7x7 channels 128/160/160/192), Mixed_7a InceptionD, Mixed_7b FIDInceptionE_1, Mixed_7c
                 FIDInceptionE_2, adaptive average pool -> [B, 2048]
    pool patches branch pool of A / C / E_1: average 3x3/1 pad 1, count_include_pad=False; of E_2: max 3x3/1 pad 1
    BasicConv2d  torchvision's: conv without bias -> BatchNorm(eps=0.001) -> ReLU

State dict keys are torchvision's Inception3 names (`Conv2d_1a_3x3.conv.weight`, `Mixed_5b.branch1x1.bn.running_var`,
...), so pytorch-fid's `pt_inception-2015-12-05-6726825d.pth` loads unchanged (`load_inception_state`; `fc.*`,
`AuxLogits.*` and `num_batches_tracked` are ignored, every trunk key is required).  Without that file the trunk is the
deterministic fill of `synthetic_state` (synth.det_normal, He-scaled): an FID on it has FID's architecture and cost,
NOT its ImageNet calibration, and is not comparable with published FID.

CPU tensors run the reference's composite form (conv -> BN -> ReLU, F.* pools, torch.cat).  Device float32 tensors
run csrc/inception.hip (op/inception.py): BatchNorm folded into weight and bias once per load / device move, every
convolution an fp32-MFMA implicit GEMM writing straight into its slice of the block's concatenated output, the 1x1
heads of a block that read the same input as one GEMM, and native pools, resize and global average — no F.conv2d,
F.interpolate, F.*pool* or torch.cat.
"""
import hashlib

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import synth
from .op import inception as _op

SYNTHETIC = "synthetic"
_IGNORED_PREFIXES = ("fc.", "AuxLogits.")


class BasicConv2d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0):
        super().__init__()
        kh, kw = (kernel_size, kernel_size) if isinstance(kernel_size, int) else kernel_size
        ph, pw = (padding, padding) if isinstance(padding, int) else padding
        self.conv = nn.Conv2d(in_channels, out_channels, (kh, kw), stride=stride, padding=(ph, pw), bias=False)
        self.bn = nn.BatchNorm2d(out_channels, eps=0.001)
        self.geom = (kh, kw, stride, ph, pw)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)

    def folded(self):
        """(weight, bias) with the BatchNorm folded in, computed in float64, rounded to float32."""
        w = self.conv.weight.detach().double()
        bn = self.bn
        scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        bias = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
        return (w * scale[:, None, None, None]).float(), bias.float()


class FIDInceptionA(nn.Module):
    def __init__(self, in_channels, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_channels, 64, 1)
        self.branch5x5_1 = BasicConv2d(in_channels, 48, 1)
        self.branch5x5_2 = BasicConv2d(48, 64, 5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, padding=1)
        self.branch_pool = BasicConv2d(in_channels, pool_features, 1)

    def forward(self, x):
        b1 = self.branch1x1(x)
        b5 = self.branch5x5_2(self.branch5x5_1(x))
        b3 = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        bp = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False))
        return torch.cat([b1, b5, b3, bp], 1)


class InceptionB(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3 = BasicConv2d(in_channels, 384, 3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, stride=2)

    def forward(self, x):
        b3 = self.branch3x3(x)
        bd = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        return torch.cat([b3, bd, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class FIDInceptionC(nn.Module):
    def __init__(self, in_channels, channels_7x7):
        super().__init__()
        c7 = channels_7x7
        self.branch1x1 = BasicConv2d(in_channels, 192, 1)
        self.branch7x7_1 = BasicConv2d(in_channels, c7, 1)
        self.branch7x7_2 = BasicConv2d(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, (7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(in_channels, c7, 1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, (1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(in_channels, 192, 1)

    def forward(self, x):
        b1 = self.branch1x1(x)
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = self.branch7x7dbl_1(x)
        for m in (self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4, self.branch7x7dbl_5):
            bd = m(bd)
        bp = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False))
        return torch.cat([b1, b7, bd, bp], 1)


class InceptionD(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(in_channels, 192, 1)
        self.branch3x3_2 = BasicConv2d(192, 320, 3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(in_channels, 192, 1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, (1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, (7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, 3, stride=2)

    def forward(self, x):
        b3 = self.branch3x3_2(self.branch3x3_1(x))
        b7 = self.branch7x7x3_1(x)
        for m in (self.branch7x7x3_2, self.branch7x7x3_3, self.branch7x7x3_4):
            b7 = m(b7)
        return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class FIDInceptionE(nn.Module):
    """FIDInceptionE_1 (pool='avg') and FIDInceptionE_2 (pool='max')."""

    def __init__(self, in_channels, pool):
        super().__init__()
        self.pool = pool
        self.branch1x1 = BasicConv2d(in_channels, 320, 1)
        self.branch3x3_1 = BasicConv2d(in_channels, 384, 1)
        self.branch3x3_2a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 448, 1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, 3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(in_channels, 192, 1)

    def forward(self, x):
        b1 = self.branch1x1(x)
        b3 = self.branch3x3_1(x)
        b3 = torch.cat([self.branch3x3_2a(b3), self.branch3x3_2b(b3)], 1)
        bd = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        bd = torch.cat([self.branch3x3dbl_3a(bd), self.branch3x3dbl_3b(bd)], 1)
        if self.pool == "avg":
            bp = F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)
        else:
            bp = F.max_pool2d(x, kernel_size=3, stride=1, padding=1)
        return torch.cat([b1, b3, bd, self.branch_pool(bp)], 1)


BLOCKS = ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a",
          "Mixed_7b", "Mixed_7c")


class InceptionV3FID(nn.Module):
    """forward(x [B, 3, H, W]) -> features [B, 2048]; forward(x, return_blocks=True) -> (features, [block 0, 1, 2
    outputs]) — the reference's InceptionV3 blocks 0 (after the first max pool, 64 channels), 1 (after the second,
    192) and 2 (after Mixed_6e, 768)."""

    def __init__(self):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, 3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, 3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, 3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, 1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, 3)
        self.Mixed_5b = FIDInceptionA(192, 32)
        self.Mixed_5c = FIDInceptionA(256, 64)
        self.Mixed_5d = FIDInceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = FIDInceptionC(768, 128)
        self.Mixed_6c = FIDInceptionC(768, 160)
        self.Mixed_6d = FIDInceptionC(768, 160)
        self.Mixed_6e = FIDInceptionC(768, 192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = FIDInceptionE(1280, "avg")
        self.Mixed_7c = FIDInceptionE(2048, "max")
        self.trunk_name = SYNTHETIC
        load_inception_state(self, synthetic_state(self))
        self.eval()
        self._folded = None

    # -- weights -----------------------------------------------------------------------------------------------------
    def _apply(self, fn, *args, **kwargs):
        self._folded = None
        return super()._apply(fn, *args, **kwargs)

    def load_weights_file(self, path):
        """Loads pytorch-fid's pt_inception-2015-12-05-6726825d.pth (or any Inception3-keyed state dict) and names
        the trunk by the file's SHA-256."""
        state = torch.load(path, map_location="cpu", weights_only=False)
        load_inception_state(self, state)
        self.trunk_name = file_sha256(path)

    # -- forward -----------------------------------------------------------------------------------------------------
    def forward(self, x, return_blocks=False):
        if x.device.type == "cuda" and x.dtype == torch.float32:
            feat, blocks = self._native(x)
        else:
            feat, blocks = self._composite(x)
        return (feat, blocks) if return_blocks else feat

    def _composite(self, x):
        if x.shape[2] != 299 or x.shape[3] != 299:
            x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
        x = self.Conv2d_2b_3x3(self.Conv2d_2a_3x3(self.Conv2d_1a_3x3(x)))
        b0 = x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = self.Conv2d_4a_3x3(self.Conv2d_3b_1x1(x))
        b1 = x = F.max_pool2d(x, kernel_size=3, stride=2)
        for name in BLOCKS[:8]:
            x = getattr(self, name)(x)
        b2 = x
        for name in BLOCKS[8:]:
            x = getattr(self, name)(x)
        return F.adaptive_avg_pool2d(x, (1, 1)).flatten(1), [b0, b1, b2]

    def _fold(self):
        """Folded GEMMs for the native path, keyed by module name; the 1x1 heads of a block concatenated along M."""
        if self._folded is not None:
            return self._folded
        out = {}

        def one(name, mods):
            ws, bs = zip(*[m.folded() for m in mods])
            kh, kw, stride, ph, pw = mods[0].geom
            dev = mods[0].conv.weight.device
            out[name] = _op.FoldedConv(torch.cat(ws, 0).to(dev), torch.cat(bs, 0).to(dev), kh, kw, stride, ph, pw)

        for name, mod in self.named_modules():
            if isinstance(mod, BasicConv2d):
                one(name, [mod])
        for name in BLOCKS:
            blk = getattr(self, name)
            heads = {FIDInceptionA: ("branch1x1", "branch5x5_1", "branch3x3dbl_1"),
                     FIDInceptionC: ("branch1x1", "branch7x7_1", "branch7x7dbl_1"),
                     InceptionD: ("branch3x3_1", "branch7x7x3_1"),
                     FIDInceptionE: ("branch1x1", "branch3x3_1", "branch3x3dbl_1")}.get(type(blk))
            if heads:
                one(name + ".heads", [getattr(blk, h) for h in heads])
        self._folded = out
        return out

    def _native(self, x):
        f = self._fold()
        conv, pool = _op.conv, _op.pool
        if x.shape[2] != 299 or x.shape[3] != 299:
            x = _op.resize299(x)
        x = conv(x, f["Conv2d_1a_3x3"])
        x = conv(x, f["Conv2d_2a_3x3"])
        x = conv(x, f["Conv2d_2b_3x3"])
        b0 = x = pool(x, "max3s2")
        x = conv(x, f["Conv2d_3b_1x1"])
        x = conv(x, f["Conv2d_4a_3x3"])
        b1 = x = pool(x, "max3s2")
        for name in BLOCKS:
            kind = type(getattr(self, name))
            x = _NATIVE_BLOCK[kind](self, f, name, x)
            if name == "Mixed_6e":
                b2 = x
        return _op.gap(x), [b0, b1, b2]

    def _block_a(self, f, name, x):
        blk = getattr(self, name)
        conv = _op.conv
        b, _, h, w = x.shape
        pf = blk.branch_pool.conv.out_channels
        out = x.new_empty(b, 224 + pf, h, w)
        t5, t3 = x.new_empty(b, 48, h, w), x.new_empty(b, 64, h, w)
        conv(x, f[name + ".heads"], [(out, 0, 0), (t5, 64, 0), (t3, 112, 0)])
        conv(t5, f[name + ".branch5x5_2"], [(out, 0, 64)])
        conv(conv(t3, f[name + ".branch3x3dbl_2"]), f[name + ".branch3x3dbl_3"], [(out, 0, 128)])
        conv(_op.pool(x, "avg3s1"), f[name + ".branch_pool"], [(out, 0, 224)])
        return out

    def _block_b(self, f, name, x):
        conv = _op.conv
        b, c, h, w = x.shape
        oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        out = x.new_empty(b, 480 + c, oh, ow)
        conv(x, f[name + ".branch3x3"], [(out, 0, 0)])
        t = conv(conv(x, f[name + ".branch3x3dbl_1"]), f[name + ".branch3x3dbl_2"])
        conv(t, f[name + ".branch3x3dbl_3"], [(out, 0, 384)])
        _op.pool(x, "max3s2", out, 480)
        return out

    def _block_c(self, f, name, x):
        blk = getattr(self, name)
        conv = _op.conv
        b, _, h, w = x.shape
        c7 = blk.branch7x7_1.conv.out_channels
        out = x.new_empty(b, 768, h, w)
        t7, td = x.new_empty(b, c7, h, w), x.new_empty(b, c7, h, w)
        conv(x, f[name + ".heads"], [(out, 0, 0), (t7, 192, 0), (td, 192 + c7, 0)])
        conv(conv(t7, f[name + ".branch7x7_2"]), f[name + ".branch7x7_3"], [(out, 0, 192)])
        for k in (2, 3, 4):
            td = conv(td, f[name + ".branch7x7dbl_%d" % k])
        conv(td, f[name + ".branch7x7dbl_5"], [(out, 0, 384)])
        conv(_op.pool(x, "avg3s1"), f[name + ".branch_pool"], [(out, 0, 576)])
        return out

    def _block_d(self, f, name, x):
        conv = _op.conv
        b, c, h, w = x.shape
        oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        out = x.new_empty(b, 512 + c, oh, ow)
        t3, t7 = x.new_empty(b, 192, h, w), x.new_empty(b, 192, h, w)
        conv(x, f[name + ".heads"], [(t3, 0, 0), (t7, 192, 0)])
        conv(t3, f[name + ".branch3x3_2"], [(out, 0, 0)])
        t7 = conv(conv(t7, f[name + ".branch7x7x3_2"]), f[name + ".branch7x7x3_3"])
        conv(t7, f[name + ".branch7x7x3_4"], [(out, 0, 320)])
        _op.pool(x, "max3s2", out, 512)
        return out

    def _block_e(self, f, name, x):
        blk = getattr(self, name)
        conv = _op.conv
        b, _, h, w = x.shape
        out = x.new_empty(b, 2048, h, w)
        t3, td = x.new_empty(b, 384, h, w), x.new_empty(b, 448, h, w)
        conv(x, f[name + ".heads"], [(out, 0, 0), (t3, 320, 0), (td, 704, 0)])
        conv(t3, f[name + ".branch3x3_2a"], [(out, 0, 320)])
        conv(t3, f[name + ".branch3x3_2b"], [(out, 0, 704)])
        td = conv(td, f[name + ".branch3x3dbl_2"])
        conv(td, f[name + ".branch3x3dbl_3a"], [(out, 0, 1088)])
        conv(td, f[name + ".branch3x3dbl_3b"], [(out, 0, 1472)])
        pooled = _op.pool(x, "avg3s1" if blk.pool == "avg" else "max3s1")
        conv(pooled, f[name + ".branch_pool"], [(out, 0, 1856)])
        return out


_NATIVE_BLOCK = {FIDInceptionA: InceptionV3FID._block_a, InceptionB: InceptionV3FID._block_b,
                 FIDInceptionC: InceptionV3FID._block_c, InceptionD: InceptionV3FID._block_d,
                 FIDInceptionE: InceptionV3FID._block_e}


# -- state dicts -----------------------------------------------------------------------------------------------------
def trunk_keys(net):
    return [k for k in net.state_dict() if not k.endswith("num_batches_tracked")]


def load_inception_state(net, state):
    """Loads a torchvision-Inception3-keyed state dict.  `fc.*`, `AuxLogits.*` and `num_batches_tracked` are
    ignored; a missing trunk key (or an unknown one) raises KeyError."""
    state = {k: v for k, v in state.items()
             if not k.startswith(_IGNORED_PREFIXES) and not k.endswith("num_batches_tracked")}
    want = trunk_keys(net)
    missing = [k for k in want if k not in state]
    unknown = sorted(set(state) - set(want))
    if missing or unknown:
        raise KeyError("Inception state dict: missing %s, unexpected %s" % (missing[:8], unknown[:8]))
    with torch.no_grad():
        own = net.state_dict()
        for k in want:
            v = torch.as_tensor(state[k])
            if tuple(v.shape) != tuple(own[k].shape):
                raise ValueError("Inception state dict: %s has shape %s, expected %s"
                                 % (k, tuple(v.shape), tuple(own[k].shape)))
            own[k].copy_(v)
    net._folded = None


def synthetic_state(net=None):
    """Deterministic torchvision-keyed stand-in for the FID weights: conv weights He-scaled det_normal, BatchNorm
    gamma ~ 1, beta / running_mean ~ 0.02, running_var ~ 1 — features of order one through all eleven blocks."""
    if net is None:
        net = InceptionV3FID()
    state, key = {}, 9000
    for name, mod in net.named_modules():
        if not isinstance(mod, BasicConv2d):
            continue
        w = mod.conv.weight
        fan_in = w[0].numel()
        m = w.shape[0]
        state[name + ".conv.weight"] = torch.from_numpy(
            synth.det_normal(tuple(w.shape), key) * np.float32(np.sqrt(2.0 / fan_in)))
        state[name + ".bn.weight"] = torch.from_numpy(1 + 0.1 * synth.det_normal((m,), key + 1))
        state[name + ".bn.bias"] = torch.from_numpy(0.02 * synth.det_normal((m,), key + 2))
        state[name + ".bn.running_mean"] = torch.from_numpy(0.02 * synth.det_normal((m,), key + 3))
        state[name + ".bn.running_var"] = torch.from_numpy(
            (1 + 0.2 * np.abs(synth.det_normal((m,), key + 4))).astype(np.float32))
        key += 5
    return state


def file_sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for chunk in iter(lambda: fh.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()


def load_inception(weights=None, device="cpu"):
    """The FID trunk on `device`: pytorch-fid's weight file when `weights` names one, else the synthetic fill."""
    net = InceptionV3FID()
    if weights:
        net.load_weights_file(weights)
    return net.to(device).eval()


# -- feature statistics ----------------------------------------------------------------------------------------------
class FeatureStats:
    """Running mean and covariance of feature rows, equal to np.mean(f, 0) and np.cov(f, rowvar=False) of all rows
    concatenated (float64).  Every batch is shifted by the first batch's mean; the sum and the Gram matrix of the
    shifted rows accumulate in float64 (device: csrc/inception.hip k_fs_*, fixed order, no atomics; CPU: numpy).
    Only `finalize()` moves anything to the host."""

    def __init__(self):
        self.count = 0
        self.dim = None
        self._dev = None
        self._sum = self._gram = self._shift = None

    def update(self, feat):
        feat = feat.detach()
        if feat.dim() != 2:
            raise ValueError("FeatureStats.update: expected [n, d] features, got %s" % (tuple(feat.shape),))
        n, d = feat.shape
        if n == 0:
            return
        if self.dim is None:
            self.dim = d
            self._dev = feat.device
            if feat.device.type == "cuda":
                kw = dict(dtype=torch.float64, device=feat.device)
                self._sum, self._gram, self._shift = torch.zeros(d, **kw), torch.zeros(d, d, **kw), torch.zeros(d, **kw)
            else:
                self._sum, self._gram = np.zeros(d), np.zeros((d, d))
                self._shift = None
        elif d != self.dim or feat.device != self._dev:
            raise ValueError("FeatureStats.update: features [*, %d] on %s expected" % (self.dim, self._dev))
        if self._dev.type == "cuda":
            _op.stats_update(self._sum, self._gram, self._shift, feat.float(), self.count == 0)
        else:
            x = feat.cpu().numpy().astype(np.float64)
            if self._shift is None:
                self._shift = x.mean(0)
            x = x - self._shift
            self._sum += x.sum(0)
            self._gram += x.T @ x
        self.count += n

    def finalize(self):
        """-> (mean [d], cov [d, d]) as float64 numpy arrays."""
        if self.count < 2:
            raise ValueError("FeatureStats.finalize: need at least two rows, have %d" % self.count)
        if self._dev.type == "cuda":
            mean, cov = _op.stats_finalize(self._sum, self._gram, self._shift, self.count)
            return mean.cpu().numpy(), cov.cpu().numpy()
        n = float(self.count)
        mean = self._shift + self._sum / n
        cov = (self._gram - np.outer(self._sum, self._sum) / n) / (n - 1)
        return mean, cov
