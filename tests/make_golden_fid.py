"""TEST INFRASTRUCTURE — writes tests/golden/fid_net.npz and tests/golden/fid_calc.npz by RUNNING THE REFERENCE's FID
Inception (inception.py) and its calc_fid (fid.py) where the reference sources lie.  Never imported by a test (the
reference does not exist on the GPU machine).  Re-run:  python tests/make_golden_fid.py

* The network is the reference's own inception.py: InceptionV3([3], normalize_input=False) (as calc_inception.
  load_patched_inception_v3 builds it) on fid_inception_v3(), with the reference's FIDInceptionA / FIDInceptionC /
  FIDInceptionE_1 / FIDInceptionE_2 classes and forwards.
* torchvision is not installed, so the torchvision pieces the reference imports are provided in memory below:
  `models.inception.Inception3`, `BasicConv2d`, `InceptionA`..`InceptionE`, `models.inception_v3` and
  `load_state_dict_from_url`.  They restate torchvision's module layout (names, channel counts, kernel sizes, paddings,
  strides, BatchNorm eps 0.001) and only the forwards the FID model does not patch: BasicConv2d, InceptionB and
  InceptionD.  Every FID patch runs from the reference's source.  (oracle/make_golden.py takes the same approach for
  torchvision's VGG16.)  `load_state_dict_from_url` returns the product's synthetic fill
  (stylerenderer_amd.inception.synthetic_state) plus a zero `fc` layer, instead of downloading the weights.
* calc_fid is the reference's fid.py function, extracted from the file and exec'ed with scipy.linalg and numpy (the
  file's module level imports the reference's model and calc_inception, which need CUDA extensions and torchvision;
  oracle/ref_shim.py provides the former, but calc_fid uses neither).
* Every network case also runs in float64 (weights and input), so the tests can measure the reference's own float32
  error and set their bars from it.  Stored per case: the 2048 features and the per-channel spatial means of blocks
  0-2 (to localise a failure), float32 and float64.  No weights and no inputs are stored (tests/fid_cases.py rebuilds
  the inputs).
"""
import io
import os
import re
import sys
import types
from contextlib import redirect_stdout

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import fid_cases  # noqa: E402
import ref_shim  # noqa: E402
from stylerenderer_amd import inception as sr_inception  # noqa: E402

OUT = os.path.join(HERE, "golden")


# ---- torchvision stand-ins: module layout + unpatched forwards ------------------------------------------------------
class BasicConv2d(nn.Module):
    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, bias=False, **kwargs)
        self.bn = nn.BatchNorm2d(out_channels, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)


class InceptionA(nn.Module):
    def __init__(self, in_channels, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(in_channels, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(in_channels, pool_features, kernel_size=1)


class InceptionB(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3 = BasicConv2d(in_channels, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        branch3x3 = self.branch3x3(x)
        branch3x3dbl = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        branch_pool = F.max_pool2d(x, kernel_size=3, stride=2)
        return torch.cat([branch3x3, branch3x3dbl, branch_pool], 1)


class InceptionC(nn.Module):
    def __init__(self, in_channels, channels_7x7):
        super().__init__()
        c7 = channels_7x7
        self.branch1x1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)


class InceptionD(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        branch3x3 = self.branch3x3_2(self.branch3x3_1(x))
        branch7x7x3 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        branch_pool = F.max_pool2d(x, kernel_size=3, stride=2)
        return torch.cat([branch3x3, branch7x7x3, branch_pool], 1)


class InceptionE(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_channels, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(in_channels, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)


class Inception3(nn.Module):
    """torchvision's Inception3 trunk layout with aux_logits=False (the only form fid_inception_v3 builds)."""

    def __init__(self, num_classes=1000, aux_logits=True, transform_input=False, **kw):
        super().__init__()
        assert not aux_logits
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, pool_features=32)
        self.Mixed_5c = InceptionA(256, pool_features=64)
        self.Mixed_5d = InceptionA(288, pool_features=64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, channels_7x7=128)
        self.Mixed_6c = InceptionC(768, channels_7x7=160)
        self.Mixed_6d = InceptionC(768, channels_7x7=160)
        self.Mixed_6e = InceptionC(768, channels_7x7=192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280)
        self.Mixed_7c = InceptionE(2048)
        self.fc = nn.Linear(2048, num_classes)


def inception_v3(pretrained=False, **kw):
    assert not pretrained
    return Inception3(**kw)


def load_state_dict_from_url(url, progress=True):
    state = sr_inception.synthetic_state()
    state["fc.weight"] = torch.zeros(1008, 2048)
    state["fc.bias"] = torch.zeros(1008)
    return state


def reference_inception():
    """The reference's inception.py imported against the stand-ins."""
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    tv_inc = mod("torchvision.models.inception", Inception3=Inception3, BasicConv2d=BasicConv2d, InceptionA=InceptionA,
                 InceptionB=InceptionB, InceptionC=InceptionC, InceptionD=InceptionD, InceptionE=InceptionE)
    tv_utils = mod("torchvision.models.utils", load_state_dict_from_url=load_state_dict_from_url)
    tvm = mod("torchvision.models", inception=tv_inc, utils=tv_utils, inception_v3=inception_v3)
    mod("torchvision", models=tvm)
    sys.path.insert(0, ref_shim.REF)
    try:
        import inception as ref_inception
    finally:
        sys.path.remove(ref_shim.REF)
    assert ref_inception.load_state_dict_from_url is load_state_dict_from_url
    return ref_inception


def reference_calc_fid():
    from scipy import linalg

    src = open(os.path.join(ref_shim.REF, "fid.py")).read().replace("\t", "    ")
    m = re.search(r"^def calc_fid\(.*?(?=^if __name__)", src, flags=re.S | re.M)
    env = {"linalg": linalg, "np": np}
    exec(m.group(0), env)
    return env["calc_fid"]


def run_net(ref_inception, dtype):
    net = ref_inception.InceptionV3([3], normalize_input=False).eval().to(dtype)
    out = {}
    with torch.no_grad():
        for name in fid_cases.NET_CASES:
            x = torch.from_numpy(fid_cases.images(name)).to(dtype)
            # the blocks of InceptionV3.forward, with the block outputs kept (resize as forward does it)
            h = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
            for k, block in enumerate(net.blocks):
                h = block(h)
                if k < 3:
                    out["%s_blk%d" % (name, k)] = h.mean((2, 3)).numpy()
            feat = net(x)[0].view(x.shape[0], -1)
            assert torch.equal(feat, h.view(x.shape[0], -1))
            out["%s_feat" % name] = feat.numpy()
    return out


def main():
    if not ref_shim.available():
        raise SystemExit("reference sources not present")
    ref_inception = reference_inception()
    net = {}
    for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        for k, v in run_net(ref_inception, dtype).items():
            net["%s_%s" % (k, tag)] = v
    for name in fid_cases.NET_CASES:
        f32, f64 = net[name + "_feat_f32"].astype(np.float64), net[name + "_feat_f64"]
        print("%s: features |f| max %.3f, reference fp32 error %.2e of scale"
              % (name, np.abs(f64).max(), np.abs(f32 - f64).max() / np.abs(f64).max()))
    np.savez_compressed(os.path.join(OUT, "fid_net.npz"), **net)

    calc_fid = reference_calc_fid()
    calc = {}
    for name in fid_cases.FID_CASES:
        s, r = fid_cases.fid_inputs(name)
        (ms, cs), (mr, cr) = fid_cases.stats(s), fid_cases.stats(r)
        buf = io.StringIO()
        with redirect_stdout(buf):
            calc[name] = np.float64(calc_fid(ms, cs, mr, cr))
        calc[name + "_eps_branch"] = np.bool_("singular" in buf.getvalue())
        print("calc_fid %s: %.9g (eps retry: %s)" % (name, calc[name], bool(calc[name + "_eps_branch"])))
    np.savez_compressed(os.path.join(OUT, "fid_calc.npz"), **calc)


if __name__ == "__main__":
    main()
