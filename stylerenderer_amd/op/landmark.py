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

Pose-aware form (landmark_loss(..., normals=, lines=, axis=, vis=); definition: `landmark_dynamic_composite`).  A detector
puts the jaw landmarks on the visible silhouette and guesses landmarks that are turned away, so
  * a contour line c = (landmark line_lmk[c], side[c] in {-1, +1}, candidate vertices cand[cand_off[c] : cand_off[c + 1]],
    candidate 0 the static vertex) replaces its landmark by the candidate furthest out across the face:
        a = (v[b, i_up] - v[b, i_down]).xy        u = (a.y, -a.x) / |a|  ((1, 0) when |a| < 1e-6)
        sel[b, c] = cand[first arg max_j side[c] dot(v[b, cand_j].xy, u)]        P_l = v[b, sel[b, c]]
    (u, the image direction across the face, turns with an in-plane roll, so a roll leaves sel unchanged);
  * every other landmark's confidence is multiplied by gate = smoothstep(clamp((m - lo) / (hi - lo), 0, 1)) of
    m = N.z / max(|N|, 1e-12), N = sum_k bary[l, k] normals[b, idx[l, k]] (hi == lo: a step at m > lo); outward normals
    with z > 0 face the camera (the rasterizer keeps the greater z).  Contour landmarks sit on the silhouette, where
    N.z ~ 0 by construction, and are not gated.
sel and gate are constants of the backward pass.  Device fp32: sr_landmark_dyn_fwd / sr_landmark_dyn_bwd, again one launch
each way.
"""
import numpy as np
import torch
from torch.autograd import Function

from ._dispatch import DerivedCache, host_array, is_device_tensor, native

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
    off, cl, cw = _csr(ih, bh, nv)
    value = (torch.from_numpy(off).to(dev), torch.from_numpy(cl).to(dev), torch.from_numpy(cw).to(dev),
             torch.from_numpy(ih.astype(np.int32)).to(dev), torch.from_numpy(bh).to(dev), idx, bary)
    return _CSR_CACHE.put(key, value)[:5]                              # (idx, bary kept alive: the key holds their addresses)


def _csr(ih, bh, nv):
    """(off int32 [nv + 1], l int32 [E], w float32 [E]) of an embedding on the host: per vertex, ascending 3 l + k."""
    flat, wflat = ih.reshape(-1), bh.reshape(-1)
    used = np.nonzero(wflat != 0)[0]
    order = used[np.argsort(flat[used], kind="stable")]
    off = np.zeros(nv + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(flat[used], minlength=nv))
    return off, (order // 3).astype(np.int32), wflat[order]


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
    native(g).sr_landmark_loss_bwd(gv, g, gr, gr.stride(0) if b > 1 else 0, off, cl, cw, b, n_l, nv, h, w,
                                   int(out is not None))
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
    native(vc).sr_landmark_loss_fwd(rows, p, g, vc, lists[3], lists[4], q, c, b, n_l, nv, h, w, float(beta),
                                    float(weight))
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


def landmark_loss(v, idx, bary, target, conf, size, beta=1.0, weight=1.0, normals=None, lines=None, axis=None, vis=None):
    """(rows [B], p [B, L, 2]) of posed vertices v [B, nv, 3] under the embedding (idx, bary) against target [B, L, 2]
    with weights conf [B, L] in an (H, W) = `size` picture (an int: square).  rows carries the gradient to v; `weight`
    scales rows (folded into the kernel: no extra launch).  On the device p is detached; from the composite it is not.
    With any of normals [B, nv, 3], lines, axis = (i_up, i_down), vis = (lo, hi) the pose-aware term runs instead
    (`landmark_loss_ex`, which also returns the selection and the gate); with all four None, the term above."""
    if not (normals is None and lines is None and axis is None and vis is None):
        return landmark_loss_ex(v, idx, bary, target, conf, size, beta, weight, normals, lines, axis, vis)[:2]
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


# ---- pose-aware landmarks: contour lines and the visibility gate -----------------------------------------------------
def check_lines(lines, n_l, nv=None):
    """The four arrays of `lines` on the host (int64): (line_lmk [C], side [C], cand_off [C + 1], cand [E]); None is no
    line at all.  Refused: a landmark outside [0, n_l) or in two lines, a side other than -1 / +1, offsets that do not
    partition cand, an empty line, and (with nv) a candidate outside [0, nv)."""
    if lines is None:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int64)
    if len(lines) != 4:
        raise ValueError("landmark_loss: lines must be (line_lmk [C], side [C], cand_off [C + 1], cand [E])")
    raw = [host_array(x).reshape(-1) for x in lines]
    if not all(np.all(np.round(a) == a) for a in raw):
        raise ValueError("landmark_loss: lines hold whole numbers")
    lm, side, off, cand = (a.astype(np.int64) for a in raw)
    n_c = len(lm)
    if len(side) != n_c or len(off) != n_c + 1:
        raise ValueError("landmark_loss: %d contour lines need side [C] and cand_off [C + 1], got %d and %d"
                         % (n_c, len(side), len(off)))
    if n_c and (lm.min() < 0 or lm.max() >= n_l):
        raise ValueError("landmark_loss: a contour line names a landmark outside [0, %d)" % n_l)
    if len(np.unique(lm)) != n_c:
        raise ValueError("landmark_loss: a landmark appears in more than one contour line")
    if not np.all(np.abs(side) == 1):
        raise ValueError("landmark_loss: the side of a contour line is -1 or +1")
    if off[0] != 0 or off[-1] != len(cand) or np.any(np.diff(off) < 0):
        raise ValueError("landmark_loss: cand_off must rise from 0 to the number of candidates")
    if np.any(np.diff(off) == 0):
        raise ValueError("landmark_loss: a contour line without candidates (an empty line)")
    if len(cand) and (cand.min() < 0 or (nv is not None and cand.max() >= nv)):
        raise ValueError("landmark_loss: a contour candidate outside the mesh's vertices%s"
                         % ("" if nv is None else " [0, %d)" % nv))
    return lm, side, off, cand


def _check_dynamic(normals, lines, axis, vis, v):
    """The refusals of the pose-aware term that do not need the lists; returns (lo, hi) or None."""
    if vis is not None:
        if normals is None:
            raise ValueError("landmark_loss: vis (the visibility gate) needs the posed normals")
        lo, hi = float(vis[0]), float(vis[1])
        if not lo <= hi:
            raise ValueError("landmark_loss: vis = (lo, hi) needs lo <= hi, got (%g, %g)" % (lo, hi))
        vis = (lo, hi)
    if lines is not None and axis is None:
        raise ValueError("landmark_loss: contour lines need axis = (i_up, i_down), the two vertices that span the face's "
                         "up direction")
    if normals is not None and tuple(normals.shape) != tuple(v.shape):
        raise ValueError("landmark_loss: normals %s must have the vertices' shape %s" % (tuple(normals.shape), tuple(v.shape)))
    return vis


def _check_axis(axis, nv):
    if axis is None:
        return 0, 0
    i_up, i_down = int(axis[0]), int(axis[1])
    if not (0 <= i_up < nv and 0 <= i_down < nv):
        raise ValueError("landmark_loss: axis vertex outside [0, %d)" % nv)
    return i_up, i_down


def across_direction(v, axis):
    """u [B, 2]: the image direction across the face of vertices v [B, nv, 3], (a.y, -a.x) / |a| of
    a = (v[i_up] - v[i_down]).xy, (1, 0) where |a| < 1e-6."""
    a = v[:, axis[0], :2] - v[:, axis[1], :2]
    n = a.norm(dim=1, keepdim=True)
    u = torch.stack((a[:, 1], -a[:, 0]), 1) / n.clamp_min(1e-30)
    return torch.where(n >= 1e-6, u, torch.tensor([1.0, 0.0], dtype=v.dtype, device=v.device).expand_as(u))


def contour_select(v, lines, axis):
    """(pos int64 [B, C], sel int64 [B, C]): for every sample and contour line the position of the selected candidate in
    its line and its vertex index; v [B, nv, 3] (any float type and device), lines as checked by `check_lines`."""
    lm, side, off, cand = lines
    n_c, b = len(lm), v.shape[0]
    if n_c == 0:
        z = torch.zeros((b, 0), dtype=torch.int64, device=v.device)
        return z, z
    with torch.no_grad():
        u = across_direction(v, axis)
        count = np.diff(off)
        width = int(count.max())
        pad = np.zeros((n_c, width), np.int64)
        live = np.arange(width)[None, :] < count[:, None]
        pad[live] = cand
        pad_t = torch.from_numpy(pad).to(v.device)
        xy = v[:, pad_t.reshape(-1), :2].view(b, n_c, width, 2)
        score = torch.from_numpy(side).to(v.device).to(v.dtype).view(1, n_c, 1) * (
            xy[..., 0] * u[:, 0].view(b, 1, 1) + xy[..., 1] * u[:, 1].view(b, 1, 1))
        score = torch.where(torch.from_numpy(live).to(v.device)[None], score, torch.full_like(score, -float("inf")))
        best = score.max(dim=2, keepdim=True).values
        where = torch.arange(width, device=v.device).view(1, 1, width).expand_as(score)
        pos = torch.where(score == best, where, torch.full_like(where, width)).min(dim=2).values     # the first maximum
        pos = torch.where(pos >= width, torch.zeros_like(pos), pos)                                  # (no finite score)
        sel = pad_t[torch.arange(n_c, device=v.device).view(1, n_c), pos]
    return pos, sel


def visibility_gate(normals, idx, bary, vis):
    """gate [B, L] of the interpolated normals (detached): smoothstep of m = N.z / max(|N|, 1e-12) between lo and hi."""
    lo, hi = vis
    with torch.no_grad():
        n = landmark_points(normals, idx, bary)
        m = n[..., 2] / n.norm(dim=-1).clamp_min(TINY)
        if hi > lo:
            t = ((m - lo) / (hi - lo)).clamp(0.0, 1.0)
            return t * t * (3.0 - 2.0 * t)
        return (m > lo).to(m.dtype)


def landmark_dynamic_composite(v, idx, bary, target, conf, size, beta=1.0, weight=1.0, normals=None, lines=None,
                               axis=None, vis=None):
    """The defining tensor algebra of the pose-aware term: (rows [B], p [B, L, 2], sel int32 [B, C], gate [B, L]).  sel
    (an index) and gate (a detached value) are constants: the gradient reaches v through P_l alone, none reaches normals."""
    h, w = _hw(size)
    vis = _check_dynamic(normals, lines, axis, vis, v)
    n_l, nv = idx.shape[0], v.shape[1]
    lm, side, off, cand = tables = check_lines(lines, n_l, nv)
    axis = _check_axis(axis, nv)
    _, sel = contour_select(v, tables, axis)
    points = landmark_points(v, idx, bary)
    gate = torch.ones(v.shape[0], n_l, dtype=v.dtype, device=v.device)
    if vis is not None:
        gate = visibility_gate(normals.detach().to(v.dtype), idx, bary, vis)
    if len(lm):
        lm_t = torch.from_numpy(lm).to(v.device)
        on_line = torch.zeros(n_l, dtype=torch.bool, device=v.device)
        on_line[lm_t] = True
        points = points.index_copy(1, lm_t, torch.gather(v, 1, sel.unsqueeze(-1).expand(-1, -1, 3)))
        gate = torch.where(on_line.view(1, -1), torch.ones_like(gate), gate)
    p = project(points, (h, w))
    rho = torch.nn.functional.smooth_l1_loss(p, target.to(p.dtype), reduction="none", beta=float(beta)).sum(-1)
    c = conf.to(p.dtype) * gate
    rows = (weight * 2.0 / max(w, h)) * (c * rho).sum(1) / c.sum(1).clamp_min(TINY)
    return rows, p, sel.to(torch.int32), gate


_DYN_CACHE = DerivedCache(16)


def dynamic_lists(idx, bary, lines, axis, nv, device=None):
    """What the pose-aware kernels read, on `device`, built on the host once per (embedding, lines, axis, nv, device) and
    checked there (every landmark, candidate and anchor index):
      off, l, w      vertex_lists' CSR of the embedding with the contour landmarks' weights dropped
      idx, bary      the contiguous embedding
      lmk_line [L]   every landmark's line, or -1
      side [C], cand_off [C + 1], cand [E]
      line_off [nv + 1], line_c [E'], line_l [E']   for every vertex the (line, landmark) pairs in which it is a
                     candidate: its first occurrence in a line only, ascending line
      (i_up, i_down), C"""
    dev = torch.device(device) if device is not None else idx.device
    raw = None if lines is None else tuple(host_array(x).reshape(-1) for x in lines)
    key = (idx.data_ptr(), bary.data_ptr(), tuple(idx.shape), idx._version, bary._version, str(idx.device),
           str(bary.device), idx.dtype, str(dev), int(nv), None if axis is None else (int(axis[0]), int(axis[1])),
           None if raw is None else tuple((str(a.dtype), a.tobytes()) for a in raw))
    hit = _DYN_CACHE.get(key)
    if hit is not None:
        return hit[0]
    ih = idx.detach().cpu().numpy().astype(np.int64)
    bh = bary.detach().cpu().numpy().astype(np.float32)
    if ih.ndim != 2 or ih.shape[1] != 3 or bh.shape != ih.shape:
        raise ValueError("landmark_loss: idx %s and bary %s must both be [L, 3]" % (tuple(idx.shape), tuple(bary.shape)))
    if ih.size and (ih.min() < 0 or ih.max() >= nv):
        raise ValueError("landmark_loss: landmark vertex index out of range [0, %d)" % nv)
    n_l = ih.shape[0]
    lm, side, off, cand = check_lines(raw, n_l, nv)
    anchors = _check_axis(axis, nv)
    n_c = len(lm)
    lmk_line = np.full(n_l, -1, np.int32)
    lmk_line[lm] = np.arange(n_c)
    static = bh.copy()
    static[lm] = 0.0
    s_off, s_l, s_w = _csr(ih, static, nv)
    # vertex -> (line, landmark): the first occurrence of a vertex in a line, ascending line
    line_of = np.repeat(np.arange(n_c), np.diff(off))
    pairs = np.unique(np.stack((cand, line_of), 1), axis=0) if len(cand) else np.zeros((0, 2), np.int64)   # sorted rows
    line_off = np.zeros(nv + 1, np.int32)
    line_off[1:] = np.cumsum(np.bincount(pairs[:, 0], minlength=nv))
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)                      # noqa: E731
    value = dict(off=t(s_off, np.int32), l=t(s_l, np.int32), w=t(s_w, np.float32), idx=t(ih, np.int32),
                 bary=t(bh, np.float32), lmk_line=t(lmk_line, np.int32), side=t(side, np.int32),
                 cand_off=t(off, np.int32), cand=t(cand, np.int32), line_off=t(line_off, np.int32),
                 line_c=t(pairs[:, 1], np.int32), line_l=t(lm[pairs[:, 1]], np.int32), axis=anchors, n_lines=n_c)
    return _DYN_CACHE.put(key, (value, idx, bary))[0]       # (idx, bary kept alive: the key holds their addresses)


def landmark_dynamic_forward(v, idx, bary, target, conf, size, beta=1.0, weight=1.0, normals=None, lines=None, axis=None,
                             vis=None):
    """(rows [B], p, g [B, L, 2], sel int32 [B, C], gate [B, L], lists = dynamic_lists) by sr_landmark_dyn_fwd (device
    fp32, no autograd)."""
    vc, q, c = v.contiguous(), target.contiguous(), conf.contiguous()
    nc = None if vis is None else normals.contiguous()
    b, nv, _ = vc.shape
    t = dynamic_lists(idx, bary, lines, axis, nv, vc.device)
    n_l, n_c = t["idx"].shape[0], t["n_lines"]
    h, w = _hw(size)
    new = lambda shape, dt=vc.dtype: torch.empty(shape, dtype=dt, device=vc.device)              # noqa: E731
    rows, p, g, sel, gate = new((b,)), new((b, n_l, 2)), new((b, n_l, 2)), new((b, n_c), torch.int32), new((b, n_l))
    lo, hi = vis if vis is not None else (0.0, 0.0)
    native(vc).sr_landmark_dyn_fwd(rows, p, g, sel, gate, vc, nc, t["idx"], t["bary"], q, c,
                                   t["lmk_line"], t["side"], t["cand_off"], t["cand"], b, n_l, n_c, nv, t["axis"][0],
                                   t["axis"][1], int(vis is not None), float(lo), float(hi), h, w, float(beta),
                                   float(weight))
    return rows, p, g, sel, gate, t


def landmark_dynamic_backward(g, g_rows, sel, lists, nv, size, out=None):
    """gv [B, nv, 3] = g_rows[b] d rows[b] / d v from g and sel of the forward, by sr_landmark_dyn_bwd; with `out` the
    result is added into it instead."""
    h, w = _hw(size)
    b, n_l = g.shape[:2]
    gr = g_rows if g_rows.dim() == 1 and g_rows.stride(0) in (0, 1) else g_rows.reshape(-1).contiguous()
    gv = torch.empty((b, nv, 3), dtype=g.dtype, device=g.device) if out is None else out
    if out is not None and (tuple(out.shape) != (b, nv, 3) or not out.is_contiguous() or out.dtype != g.dtype):
        raise ValueError("landmark_dynamic_backward: out must be a contiguous float32 [B, nv, 3]")
    t = lists
    native(g).sr_landmark_dyn_bwd(gv, g, gr, gr.stride(0) if b > 1 else 0, sel, t["off"], t["l"], t["w"], t["line_off"],
                                  t["line_c"], t["line_l"], b, n_l, t["n_lines"], nv, h, w, int(out is not None))
    return gv


class _LandmarkDynamic(Function):
    @staticmethod
    def forward(ctx, v, idx, bary, target, conf, size, beta, weight, normals, lines, axis, vis):
        rows, p, g, sel, gate, t = landmark_dynamic_forward(v, idx, bary, target, conf, size, beta, weight, normals, lines,
                                                            axis, vis)
        saved = [g, sel, v, target, conf] + ([normals] if normals is not None else [])
        ctx.save_for_backward(*saved)
        ctx.lists, ctx.emb, ctx.lines, ctx.axis, ctx.vis = t, (idx, bary), lines, axis, vis
        ctx.nv, ctx.size, ctx.beta, ctx.weight = v.shape[1], size, float(beta), float(weight)
        ctx.mark_non_differentiable(p, sel, gate)
        ctx.set_materialize_grads(False)
        return rows, p, sel, gate

    @staticmethod
    def backward(ctx, g_rows, _gp, _gs, _gg):
        if g_rows is None:
            return (None,) * 12
        g, sel, v, q, c = ctx.saved_tensors[:5]
        if torch.is_grad_enabled():
            # a recorded backward (create_graph=True): the VJP re-derived from the composite on the saved input
            normals = ctx.saved_tensors[5] if len(ctx.saved_tensors) > 5 else None
            idx, bary = (t.to(v.device) for t in ctx.emb)
            rows = landmark_dynamic_composite(v, idx, bary, q, c, ctx.size, ctx.beta, ctx.weight, normals, ctx.lines,
                                              ctx.axis, ctx.vis)[0]
            (gv,) = torch.autograd.grad(rows, v, g_rows, create_graph=True)
            return (gv,) + (None,) * 11
        return (landmark_dynamic_backward(g, g_rows, sel, ctx.lists, ctx.nv, ctx.size),) + (None,) * 11


def landmark_loss_ex(v, idx, bary, target, conf, size, beta=1.0, weight=1.0, normals=None, lines=None, axis=None,
                     vis=None):
    """landmark_loss's pose-aware term with everything it computes: (rows [B], p [B, L, 2], sel int32 [B, C], gate
    [B, L]); sel[b, c] is the vertex contour line c selected, gate the factor on every landmark's confidence (1 for contour
    landmarks and without vis).  normals [B, nv, 3] are the posed vertex normals (needed for vis only; no gradient),
    lines = (line_lmk [C], side [C], cand_off [C + 1], cand [E]) (face_model.contour_lines), axis = (i_up, i_down) the
    vertices that span the face's up direction (needed with lines), vis = (lo, hi) or None.  Keep `lines` on the host
    (numpy arrays or CPU tensors): their bytes are part of the key under which the device lists are cached, so device
    tensors would be copied back on every call, which a graph capture refuses."""
    h, w = _hw(size)
    if v.dim() != 3 or v.shape[2] != 3:
        raise ValueError("landmark_loss: v must be [B, nv, 3], got %s" % (tuple(v.shape),))
    b, n_l = v.shape[0], idx.shape[0]
    if tuple(target.shape) != (b, n_l, 2) or tuple(conf.shape) != (b, n_l):
        raise ValueError("landmark_loss: %d samples and %d landmarks need target [B, L, 2] and conf [B, L], got %s and %s"
                         % (b, n_l, tuple(target.shape), tuple(conf.shape)))
    if float(beta) < 0:
        raise ValueError("landmark_loss: beta must not be negative")
    vis = _check_dynamic(normals, lines, axis, vis, v)
    if lines is not None:
        lines = tuple(lines)
    native = native_ok(v, target, conf) and not (target.requires_grad or conf.requires_grad)
    if native and vis is not None:
        native = is_device_tensor(normals) and normals.dtype == torch.float32
    if native:
        return _LandmarkDynamic.apply(v, idx, bary, target, conf, (h, w), float(beta), float(weight),
                                      None if vis is None else normals.detach(), lines, axis, vis)
    return landmark_dynamic_composite(v, idx.to(v.device), bary.to(v.device), target, conf, (h, w), beta, weight,
                                      normals, lines, axis, vis)
