"""Landmark reprojection term of face reconstruction: the distance between the landmarks of the posed mesh, projected to
the picture, and target landmarks read from a file (csrc/landmark.hip).

A landmark is a barycentric combination of up to three vertices, idx int32 [L, 3] and bary float32 [L, 3]
(face_model.landmark_embedding; a plain vertex is idx = (i, i, i), bary = (1, 0, 0)).  For sample b and landmark l

    P_l     = sum_k bary[l, k] v[b, idx[l, k], :]
    p_l     = ((1 + P_l.x) W / 2 - 1/2, (1 - P_l.y) H / 2 - 1/2)   the rasterizer's pixel index coordinates (reference
                                                                   op/rasterize.h:21-22, orthographic)
    e_l     = p_l - target[b, l]                                   target landmarks in the same coordinates
    rho(e)  = smooth_l1(e, beta) per coordinate                    torch's function; beta 1.0 = one pixel (reference
                                                                   train.py:329)
    rows[b] = weight (2 / max(W, H)) sum_l c[b, l] (rho(e_l.x) + rho(e_l.y)) / max(sum_l c[b, l], TINY)

c = conf [B, L] >= 0 weighs the landmarks, 0 means missing; a row of zeros gives rows[b] = 0 and a zero gradient.

Device fp32: one launch forward (p, d rows / d p and rows; fixed-order sums) and one backward (a gather over all B nv
vertices through a CSR list built once per embedding on the host: dense gradient, no memset, no scatter, no atomics, so
reruns are bit-identical); p carries no gradient.  CPU tensors and float64 take `landmark_composite`, the definition the
kernels are tested against; so does a backward pass that is itself recorded (create_graph=True: second order).
"""
import numpy as np
import torch
from torch.autograd import Function

from .. import _lib
from ._dispatch import DerivedCache, is_device_tensor, on_device_of, stream_of

TINY = 1e-12


def project(P, size):
    """[..., 3] (or [..., 2]) model coordinates -> [..., 2] pixel index coordinates of an (H, W) picture."""
    h, w = _hw(size)
    return torch.stack(((1 + P[..., 0]) * (w / 2) - 0.5, (1 - P[..., 1]) * (h / 2) - 0.5), -1)


def landmark_points(v, idx, bary):
    """P [B, L, 3] of vertices v [B, nv, 3]."""
    i = idx.long()
    return sum(bary[:, k].to(v.dtype).view(1, -1, 1) * v[:, i[:, k]] for k in range(3))


def landmark_composite(v, idx, bary, target, conf, size, beta=1.0, weight=1.0):
    """The defining tensor algebra: (rows [B], p [B, L, 2])."""
    h, w = _hw(size)
    p = project(landmark_points(v, idx, bary), (h, w))
    rho = torch.nn.functional.smooth_l1_loss(p, target.to(p.dtype), reduction="none", beta=float(beta)).sum(-1)
    c = conf.to(p.dtype)
    rows = (weight * 2.0 / max(w, h)) * (c * rho).sum(1) / c.sum(1).clamp_min(TINY)
    return rows, p


def _hw(size):
    if isinstance(size, (tuple, list)):
        return int(size[0]), int(size[1])
    return int(size), int(size)


# ---- the CSR list of an embedding: vertex -> its (landmark, weight) entries in ascending 3 l + k ----------------------
_CSR_CACHE = DerivedCache(16)


def vertex_lists(idx, bary, nv, device=None):
    """(off int32 [nv + 1], l int32 [E], w float32 [E], idx int32 [L, 3], bary float32 [L, 3]) on `device` (default:
    idx's; the embedding itself may live anywhere, face_model.landmark_embedding's is on the host): the contiguous
    embedding and, for every vertex, the landmarks that use it with a non-zero weight.  Built on the host once per
    embedding and device (cached per tensor) and checked there: every index in [0, nv)."""
    dev = torch.device(device) if device is not None else idx.device
    key = (idx.data_ptr(), bary.data_ptr(), tuple(idx.shape), idx._version, bary._version, str(idx.device),
           str(bary.device), idx.dtype, str(dev), int(nv))
    hit = _CSR_CACHE.get(key)
    if hit is not None:
        return hit[:5]
    ih = idx.detach().cpu().numpy().astype(np.int64)
    bh = bary.detach().cpu().numpy().astype(np.float32)
    if ih.ndim != 2 or ih.shape[1] != 3 or bh.shape != ih.shape:
        raise ValueError("landmark_loss: idx %s and bary %s must both be [L, 3]" % (tuple(idx.shape), tuple(bary.shape)))
    if ih.size and (ih.min() < 0 or ih.max() >= nv):
        raise ValueError("landmark_loss: landmark vertex index out of range [0, %d)" % nv)
    flat, wflat = ih.reshape(-1), bh.reshape(-1)
    used = np.nonzero(wflat != 0)[0]
    order = used[np.argsort(flat[used], kind="stable")]                # per vertex: ascending 3 l + k
    off = np.zeros(nv + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(flat[used], minlength=nv))
    value = (torch.from_numpy(off).to(dev), torch.from_numpy((order // 3).astype(np.int32)).to(dev),
             torch.from_numpy(wflat[order]).to(dev), torch.from_numpy(ih.astype(np.int32)).to(dev),
             torch.from_numpy(bh).to(dev), idx, bary)                  # idx, bary kept alive: the key holds their addresses
    return _CSR_CACHE.put(key, value)[:5]


def landmark_backward(g, g_rows, lists, nv, size, out=None):
    """gv [B, nv, 3] = g_rows[b] d rows[b] / d v from g [B, L, 2] of the forward (device fp32), by the gather kernel;
    with `out` the result is added into it instead (the kernel's accumulate flag: no separate add)."""
    off, cl, cw = lists[:3]
    h, w = _hw(size)
    b, n_l = g.shape[:2]
    gr = g_rows if g_rows.dim() == 1 and g_rows.stride(0) in (0, 1) else g_rows.reshape(-1).contiguous()
    gv = torch.empty((b, nv, 3), dtype=g.dtype, device=g.device) if out is None else out
    if out is not None and (tuple(out.shape) != (b, nv, 3) or not out.is_contiguous() or out.dtype != g.dtype):
        raise ValueError("landmark_backward: out must be a contiguous float32 [B, nv, 3]")
    with on_device_of(g):
        _lib.check(_lib.lib().sr_landmark_loss_bwd(_lib.ptr(gv), _lib.ptr(g), _lib.ptr(gr), gr.stride(0) if b > 1 else 0,
                                                   _lib.ptr(off), _lib.ptr(cl), _lib.ptr(cw), b, n_l, nv, h, w,
                                                   int(out is not None), stream_of(g)), "sr_landmark_loss_bwd")
    return gv


def landmark_forward(v, idx, bary, target, conf, size, beta=1.0, weight=1.0):
    """(rows [B], p [B, L, 2], g [B, L, 2] = d rows[b] / d p, lists = vertex_lists) by the forward kernel (device fp32,
    no autograd): what the node's forward runs and `landmark_backward` takes."""
    vc, q, c = v.contiguous(), target.contiguous(), conf.contiguous()
    b, nv, _ = vc.shape
    lists = vertex_lists(idx, bary, nv, vc.device)           # (everything the kernels read is on v's device)
    n_l = lists[3].shape[0]
    h, w = _hw(size)
    rows = torch.empty((b,), dtype=vc.dtype, device=vc.device)
    p = torch.empty((b, n_l, 2), dtype=vc.dtype, device=vc.device)
    g = torch.empty_like(p)
    ptr = _lib.ptr
    with on_device_of(vc):
        _lib.check(_lib.lib().sr_landmark_loss_fwd(ptr(rows), ptr(p), ptr(g), ptr(vc), ptr(lists[3]), ptr(lists[4]),
                                                   ptr(q), ptr(c), b, n_l, nv, h, w, float(beta), float(weight),
                                                   stream_of(vc)), "sr_landmark_loss_fwd")
    return rows, p, g, lists


class _LandmarkLoss(Function):
    @staticmethod
    def forward(ctx, v, idx, bary, target, conf, size, beta, weight):
        rows, p, g, lists = landmark_forward(v, idx, bary, target, conf, size, beta, weight)
        nv, q, c = v.shape[1], target, conf
        ctx.save_for_backward(g, *lists, v, q, c)
        ctx.nv, ctx.size, ctx.beta, ctx.weight = nv, size, float(beta), float(weight)
        ctx.mark_non_differentiable(p)
        ctx.set_materialize_grads(False)                     # (no zero-filled gradient of p made for every backward)
        return rows, p

    @staticmethod
    def backward(ctx, g_rows, _gp):
        if g_rows is None:
            return (None,) * 8
        g, off, cl, cw, idx, bary, v, q, c = ctx.saved_tensors
        if torch.is_grad_enabled():
            # the backward is itself being recorded (create_graph=True): the VJP re-derived from the composite on the
            # saved input, so that it stays differentiable in v and in g_rows
            rows, _ = landmark_composite(v, idx, bary, q, c, ctx.size, ctx.beta, ctx.weight)
            (gv,) = torch.autograd.grad(rows, v, g_rows, create_graph=True)
            return (gv,) + (None,) * 7
        return (landmark_backward(g, g_rows, (off, cl, cw), ctx.nv, ctx.size),) + (None,) * 7


def native_ok(v, target, conf):
    """The kernels take device fp32 and give first order only."""
    return all(is_device_tensor(t) and t.dtype == torch.float32 for t in (v, target, conf))


def landmark_loss(v, idx, bary, target, conf, size, beta=1.0, weight=1.0):
    """(rows [B], p [B, L, 2]) of posed vertices v [B, nv, 3] under the embedding (idx, bary) against target [B, L, 2]
    with weights conf [B, L] in an (H, W) = `size` picture (an int: square).  rows carries the gradient to v; `weight`
    scales rows (folded into the kernel: no extra launch).  On the device p is detached; from the composite it is not."""
    h, w = _hw(size)
    if v.dim() != 3 or v.shape[2] != 3:
        raise ValueError("landmark_loss: v must be [B, nv, 3], got %s" % (tuple(v.shape),))
    b, n_l = v.shape[0], idx.shape[0]
    if tuple(target.shape) != (b, n_l, 2) or tuple(conf.shape) != (b, n_l):
        raise ValueError("landmark_loss: %d samples and %d landmarks need target [B, L, 2] and conf [B, L], got %s and %s"
                         % (b, n_l, tuple(target.shape), tuple(conf.shape)))
    if float(beta) < 0:
        raise ValueError("landmark_loss: beta must not be negative")
    if native_ok(v, target, conf) and not (target.requires_grad or conf.requires_grad):
        return _LandmarkLoss.apply(v, idx, bary, target, conf, (h, w), float(beta), float(weight))
    return landmark_composite(v, idx.to(v.device), bary.to(v.device), target, conf, (h, w), beta, weight)
