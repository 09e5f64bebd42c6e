"""Adaptive discriminator augmentation kernels (C ABI sr_ada_params / sr_ada_apply / sr_ada_apply_grad / sr_ada_update,
csrc/augment.hip).

    draws(batch, device)                         one torch.randn [B, 11]: pose 5, colour 5, select 1 (standard normals;
                                                 the uniform slots are mapped through Phi in the kernel)
    params(draws, h, w, p, pose_p, color_p)      -> record [B, 28]: affine map (fp64), 3x4 colour matrix, select bit
    apply(img, rec)                              the augmented batch; differentiable in img to any order
    augment(img, p, pose_p, color_p)             draws -> params -> apply                 reference utils_3d.py:350-359
    update(state, stat, target, length)          the ADA p controller on the device       reference train.py:269-280

Device float32 [B, 3, H, W] images only: utils_3d.augment keeps the composite torch form for everything else, and that
form (with the same draws) is what the GPU tests compare against.  `p` is a Python float or a 0-d device tensor
(read by the kernel: nothing goes to the host, so the whole chain records into a graph).
"""
import ctypes

import torch
from torch.autograd import Function

from ._dispatch import native, require_f32

NDRAW = 11
REC = 28
POSE_P = (.1, .1, .05, .15, 0., .5)
COLOR_P = (.2, .3, 0., .15, .5)
# record layout (include/stylerenderer_amd.h): the affine map as six float64 in the first 12 floats
AFFINE, COLOR, SELECT = slice(0, 12), slice(12, 24), 24


def _sigmas(p, n):
    vals = [abs(float(x)) for x in torch.as_tensor(p, dtype=torch.float32).reshape(-1)[:n].tolist()]
    return (ctypes.c_float * n)(*(vals + [0.0] * (n - len(vals))))


def draws(batch, device):
    return torch.randn(batch, NDRAW, device=device)


def params(raw, h, w, p, pose_p=POSE_P, color_p=COLOR_P):
    """raw [B, 11] float32 device draws -> record [B, 28]."""
    require_f32(raw, "ada params")
    raw = raw.contiguous()
    if raw.dim() != 2 or raw.shape[1] != NDRAW:
        raise ValueError("ada params: expected draws [B, %d], got %s" % (NDRAW, tuple(raw.shape)))
    rec = torch.empty(raw.shape[0], REC, dtype=torch.float32, device=raw.device)
    p_dev, p_host = None, 0.0
    if isinstance(p, torch.Tensor):
        if p.device != raw.device or p.numel() != 1:
            raise ValueError("ada params: p must be a Python float or a one-element tensor on the images' device")
        p_dev = p.reshape(()) if p.dtype == torch.float64 else p.reshape(()).to(torch.float64)
    else:
        p_host = float(p)
    native(raw).sr_ada_params(rec, raw, raw.shape[0], _sigmas(pose_p, 6), _sigmas(color_p, 5), p_dev, p_host, h, w)
    return rec


def _launch_apply(x, rec, with_bias):
    x = x.contiguous()
    out = torch.empty_like(x)
    b, _, h, w = x.shape
    native(x).sr_ada_apply(out, x, rec, b, h, w, with_bias)
    return out


def _launch_grad(g, rec):
    g = g.contiguous()
    out = torch.empty_like(g)
    b, _, h, w = g.shape
    native(g).sr_ada_apply_grad(out, g, rec, b, h, w)
    return out


class _AdaApply(Function):
    """x -> L x (+ c): L = colour matrix . bilinear resampling per selected sample, identity otherwise."""

    @staticmethod
    def forward(ctx, x, rec, with_bias):
        ctx.save_for_backward(rec)
        return _launch_apply(x, rec, 1 if with_bias else 0)

    @staticmethod
    def backward(ctx, g):
        (rec,) = ctx.saved_tensors
        return _AdaApplyT.apply(g, rec), None, None


class _AdaApplyT(Function):
    """g -> L^T g, whose own adjoint is L again (the bias-free forward): every order of derivative stays native."""

    @staticmethod
    def forward(ctx, g, rec):
        ctx.save_for_backward(rec)
        return _launch_grad(g, rec)

    @staticmethod
    def backward(ctx, gg):
        (rec,) = ctx.saved_tensors
        return _AdaApply.apply(gg, rec, False), None


def _check_images(img):
    require_f32(img, "ada apply")
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError("ada apply: expected [B, 3, H, W], got %s" % (tuple(img.shape),))


def apply(img, rec, with_bias=True):
    _check_images(img)
    if rec.dtype != torch.float32 or tuple(rec.shape) != (img.shape[0], REC) or rec.device != img.device:
        raise ValueError("ada apply: record must be float32 [B, %d] on the images' device" % REC)
    return _AdaApply.apply(img, rec.contiguous(), with_bias)


def apply_grad(g, rec):
    """L^T g (the adjoint of the bias-free map), as a differentiable function of g."""
    _check_images(g)
    return _AdaApplyT.apply(g, rec.contiguous())


def augment(img, p, pose_p=POSE_P, color_p=COLOR_P, return_record=False):
    """Per sample, with probability p: random 2-D pose then random colour.  Three launches: the draw, the record, the
    resampling."""
    _check_images(img)
    rec = params(draws(img.shape[0], img.device), img.shape[2], img.shape[3], p, pose_p, color_p)
    out = apply(img, rec)
    return (out, rec) if return_record else out


def update_composite(state, stat, target, length):
    """The controller in torch fp64 operations, no host read (CPU tensors; the oracle of sr_ada_update)."""
    acc = state[:2] + stat.to(torch.float64)
    n = acc[1]
    hit = n > 255
    rt = acc[0] / n
    sign = torch.where(rt > target, torch.ones_like(rt), -torch.ones_like(rt))
    v = state[2] + ((sign * target) / length) * n
    v = torch.where(v > 0, v, torch.zeros_like(v))
    v = torch.where(v < 1, v, torch.ones_like(v))
    new = torch.stack([torch.where(hit, torch.zeros_like(n), acc[0]), torch.where(hit, torch.zeros_like(n), n),
                       torch.where(hit, v, state[2]), torch.where(hit, rt, state[3])])
    with torch.no_grad():
        state.copy_(new)
    return state


def update(state, stat, target, length):
    """state [4] fp64 = {sum sign D(real), count, p, r_t} <- one iteration's stat [2] (sign sum, count): in place."""
    if state.dtype != torch.float64 or state.numel() != 4 or stat.numel() != 2:
        raise ValueError("ada update: expected state float64 [4] and stat [2]")
    if not state.is_cuda:
        return update_composite(state, stat, float(target), float(length))
    st = stat if stat.dtype == torch.float32 else stat.to(torch.float32)
    native(state).sr_ada_update(state, st.contiguous(), float(target), float(length))
    return state


def composite_from_draws(img, raw, p, pose_p=POSE_P, color_p=COLOR_P):
    """The composite `augment` (utils_3d) fed with the native draws raw [B, 11], in img's dtype and on img's device:
    what sr_ada_params + sr_ada_apply compute, as grid_sample and matmul (the oracle of the GPU tests)."""
    from .. import utils_3d

    r = raw.to(dtype=img.dtype, device=img.device)
    ps = torch.as_tensor(list(_sigmas(pose_p, 6)), dtype=torch.float32).to(img.dtype).to(img.device)
    cs = torch.as_tensor(list(_sigmas(color_p, 5)), dtype=torch.float32).to(img.dtype).to(img.device)

    def phi(x):
        return 0.5 * torch.special.erfc(-x * 0.7071067811865476)

    z_pose = torch.stack([r[:, 0] * ps[0], r[:, 1] * ps[1], r[:, 2] * ps[2], ps[4] + r[:, 3] * ps[3], phi(r[:, 4])], 1)
    z_color = torch.stack([r[:, 5] * cs[0], r[:, 6] * cs[1], phi(r[:, 7]), r[:, 8] * cs[3], r[:, 9] * cs[4]], 1)
    pick = phi(r[:, 10]).view(-1, 1, 1, 1)
    return utils_3d._augment_from_draws(img, z_pose.cpu(), z_color.cpu(), pick, p, pose_p, color_p)
