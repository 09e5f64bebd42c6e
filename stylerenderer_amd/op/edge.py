"""Differentiable silhouettes: analytic antialiasing at occlusion boundaries (csrc/edge.hip).

The rasterizer's coverage is a step: a vertex moves a picture only through the barycentric weights of the pixels its
triangle already owns, so nothing image-space can pull an outline.  `antialias` blends the two pixels on either side of a
silhouette edge by how far the edge reaches past the midpoint between their centres; the blend weight is a smooth function
of the edge's two projected vertices, which gives a gradient to exactly the vertices that form the outline.

  adjacency(tri, nv) -> opp int32 [nf, 3]
      opp[f, k] is the vertex opposite edge k of face f (edge k joins corners k and (k + 1) mod 3) in the one other face that
      uses that edge; -1 for a boundary edge; -2 for an edge that more than two faces or a degenerate face (two equal
      corners) use: such an edge is never a silhouette.  Built on the host once per topology tensor, checked there (every
      index in [0, nv)), cached and pinned like op.rasterize.incidence.
  face_map(v, tri, size) -> (face int32 [B, H, W], zbuf [B, H, W])
      the rasterizer's forward in the pixels `landmark.project(., (H, W))` means: the face under every pixel (-1 where
      there is none) and the z-buffer (greater z is nearer, -FLT_MAX is empty).  The mesh is drawn with its corners exploded
      (vertex 3 f + k is corner k of face f), so the face is the winning vertex number // 3.  A non-square size is drawn in
      a square of side max(H, W) and cropped, as texture.uv_map and depth_buffer do.  No gradient; host and device results
      are equal (the rasterizer's parity).
  antialias(image [B, C, H, W], v [B, nv, 3], tri, face=None, zbuf=None, opp=None) -> out [B, C, H, W]
      Every step one operation of the tensors' float type, in this order, no fused multiply-add, quotients correctly
      rounded.  Pixel coordinates of a vertex (x, y, z):
          X = (1 + x) (W / 2) - 0.5;   Y = (1 - y) (H / 2) - 0.5
      A pair is a pixel p and its right (horizontal pair) or lower (vertical pair) neighbour q, both in the picture.  It is
      active iff face[p] != face[q].  The foreground a is q when face[p] < 0, p when face[q] < 0, otherwise q iff
      z[q] > z[p] (on equal z: p); o is the other pixel and F = face[a].  For the edges k = 0, 1, 2 of F in that order,
      with corners i = k, j = (k + 1) mod 3, own = (k + 2) mod 3, u the coordinate along the pair's axis and s the other
      coordinate minus a's:
          crossing     (s_i < 0) != (s_j < 0)
                       den = s_i - s_j;  t = s_i / den;  du = u_j - u_i;  c = u_i + du t
                       d = c - a_u when a is p (o on the positive side), a_u - c when a is q;  taken iff 0 <= d <= 1
          silhouette   opp[F, k] == -1; never for -2; otherwise with e = P_j - P_i
                       c_own = e.x (Y_own - Y_i) - e.y (X_own - X_i);  c_opp = e.x (Y_opp - Y_i) - e.y (X_opp - X_i)
                       unless (c_own > 0 and c_opp < 0) or (c_own < 0 and c_opp > 0)
      The first k that crosses and is a silhouette is the pair's edge; a pair without one contributes nothing.
          d >= 0.5:  w = d - 0.5 and o receives w (image[a] - image[o])
          d <  0.5:  w = 0.5 - d and a receives w (image[o] - image[a])
      out[p] = image[p] plus what p receives from its up to four pairs, added in the order left, right, upper, lower.
      Comparisons with NaN are false, so a NaN vertex switches its pairs off; a picture where nothing or everything is
      covered comes back bit for bit.  z decides only which pixel of a pair is in front: it gets exactly 0.
      backward, g the incoming gradient:
          gimage[p] = g[p], then per pair in the same order:  - w g[p] where p receives,  + w g[n] where the neighbour n does
          per pair with receiver r:  gd = the sum from 0, in channel order, of g[r] (image[a] - image[o])
              gsd = gd when a is p, -gd when a is q
              gu_i = gsd (1 - t);  gu_j = gsd t;  q = (gsd du) / (den den);  gs_i = -(q s_j);  gs_j = q s_i
              gx = gX (W / 2);  gy = gY (-(H / 2))                 X is u in a horizontal pair and s in a vertical one
          gc [B, 3 nf, 3], the gradient of the exploded corners (z = 0): corner (F, i) and (F, j) receive their pair's terms.
          The sum of a face's terms has a fixed order: the pixels p of the face's bounding box (floor of the least, ceil of
          the greatest corner coordinate, grown by one pixel, clipped to the picture; pixel n = row-major number in the
          box) in ascending n, right pair before lower pair; a box of more than BIG pixels is summed in 64 lanes, lane l
          adding the pixels l, l + 64, ... in that order, then lane l adds lane l + 32, 16, 8, 4, 2, 1.  A pair outside its
          face's box and a face with a non-finite corner add nothing.
          gv = texture.explode's adjoint of gc: the ordered sum over op.rasterize.incidence(tri, nv).
  coverage(v, tri, size) -> alpha [B, H, W]: `antialias` of the hard cover as a one-channel 0 / 1 image.

CPU tensors and float64 take the torch composite below, which is the definition: an autograd node whose backward is the
stated formulas in torch operations, the ordered sums included.  Float32 device tensors take sr_edge_aa_fwd /
sr_edge_aa_bwd_image / sr_edge_aa_bwd_corner and sr_explode_bwd through the C ABI: out, gimage and gv are the host float32
composite's bit for bit (for gv the first of the two rules: a host float32 definition that sums in the kernel's order).
No launch allocates, reads back or needs a zeroed buffer, so all can be captured.  Under SR_STRICT_NATIVE=1 a device tensor
the kernels do not take (float64) raises.

Not built: silhouette edges against the picture's border (a pair needs both pixels), sub-pixel edges that cross no
centre-to-centre segment, a gradient to z, and a perspective-correct crossing under the camera (the node sees the
projected mesh v', for which it is exact).
"""
import numpy as np
import torch

from ._dispatch import DerivedCache, is_device_tensor, native, strict_native
from .landmark import _hw
from .texture import _TOPO_CACHE, _div, _ordered_sum, _square_vertices

BIG = 256                             # sr_edge_big_pixels(): box pixels above which a face is summed by its wave
WAVE = 64

_ADJ_CACHE = DerivedCache(16)


# ---- topology ----------------------------------------------------------------------------------------------------------
def adjacency_host(tri, nv):
    """opp int32 [nf, 3] (numpy) of tri [nf, 3] (numpy int64): the definition of `adjacency`."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    nf = tri.shape[0]
    if tri.size and (tri.min() < 0 or tri.max() >= nv):
        raise ValueError("adjacency: vertex index out of range [0, %d)" % nv)
    opp = np.full((nf, 3), -1, np.int32)
    if nf == 0:
        return opp
    i, j = tri, tri[:, [1, 2, 0]]
    key = (np.minimum(i, j) * int(nv) + np.maximum(i, j)).reshape(-1)            # entry 3 f + k
    own = tri[:, [2, 0, 1]].reshape(-1)                                          # the corner opposite edge k
    uniq, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    start = np.concatenate(([0], np.cumsum(counts)[:-1]))
    out = np.full(3 * nf, -1, np.int64)
    two = counts[inv] == 2
    first, second = order[start[inv]], order[np.minimum(start[inv] + 1, order.shape[0] - 1)]
    other = np.where(first == np.arange(3 * nf), second, first)
    out[two] = own[other[two]]
    bad = counts > 2
    degenerate = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 2] == tri[:, 0])
    bad[inv.reshape(nf, 3)[degenerate].reshape(-1)] = True
    out[bad[inv]] = -2
    return out.reshape(nf, 3).astype(np.int32)


def adjacency(tri, nv):
    """opp int32 [nf, 3] on tri's device (the module's note); cached per topology tensor."""
    if tri.dim() != 2 or tri.shape[1] != 3 or tri.dtype != torch.int64:
        raise ValueError("adjacency: tri must be int64 [nf, 3], got %s %s" % (tri.dtype, tuple(tri.shape)))
    key = (tri.data_ptr(), tuple(tri.shape), tri._version, str(tri.device), int(nv))
    hit = _ADJ_CACHE.get(key)
    if hit is not None:
        return hit[0]
    opp = torch.from_numpy(adjacency_host(tri.detach().cpu().numpy(), int(nv))).to(tri.device).contiguous()
    _ADJ_CACHE.put(key, (opp, tri))                                              # holds `tri`: the key is its address
    return opp


def face_map(v, tri, size):
    """(face int32 [B, H, W], zbuf [B, H, W]) of the posed mesh v [B, nv, 3], tri int64 [nf, 3] (the module's note)."""
    from .rasterize import forward_with_depth

    h, w = _hw(size)
    if h < 1 or w < 1:
        raise ValueError("face_map: size must be positive, got (%d, %d)" % (h, w))
    if v.dim() != 3 or v.shape[2] != 3 or tri.dim() != 2 or tri.shape[1] != 3 or tri.dtype != torch.int64:
        raise ValueError("face_map: v [B, nv, 3] and tri int64 [nf, 3], got %s and %s" % (tuple(v.shape), tuple(tri.shape)))
    with torch.no_grad():
        v = v.detach()
        dev, nf = v.device, int(tri.shape[0])
        if h != w:
            x, y = _square_vertices(v[..., 0], v[..., 1], (h, w))
            v = torch.stack((x, y, v[..., 2]), -1)
        corners = v[:, tri.to(dev).reshape(-1)].contiguous()
        topo = _TOPO_CACHE.get((nf, str(dev)))
        if topo is None:
            topo = _TOPO_CACHE.put((nf, str(dev)), torch.arange(3 * nf, dtype=torch.int64, device=dev).view(nf, 3))
        s = max(h, w)
        index, coeff, zbuf = forward_with_depth(corners, topo, s, s)
        index, coeff, zbuf = index[:, :h, :w], coeff[:, :h, :w], zbuf[:, :h, :w]
        covered = (coeff != 0).any(-1)
        # (the rasterizer numbers the vertices of row r from r 3 nf on)
        first = torch.arange(int(v.shape[0]), device=dev).view(-1, 1, 1) * (3 * nf)
        face = torch.div(index[..., 0] - first, 3, rounding_mode="floor")
        face = torch.where(covered, face, torch.full_like(face, -1)).to(torch.int32)
        return face.contiguous(), zbuf.contiguous()


# ---- the definition ----------------------------------------------------------------------------------------------------
def pixel_coordinates(v, size):
    """(X, Y) [B, nv, 2] of v [B, nv, 3] in an (H, W) picture: three operations each."""
    h, w = _hw(size)
    return torch.stack(((1 + v[..., 0]) * (w / 2) - 0.5, (1 - v[..., 1]) * (h / 2) - 0.5), -1)


def analyse(P, tri, opp, face, zbuf, horiz):
    """The pairs of one orientation, dense over the pair grid [B, H, W - 1] (horiz) or [B, H - 1, W]: a dict with hit,
    a_is_p, recv_is_q (bool), F, k (int64), d, w, t, den, du, si, sj (P's float type; meaningful where hit) and XY
    [..., 3, 2], the pixel coordinates of F's corners."""
    b, h, w = face.shape
    nv, nf = int(P.shape[1]), int(tri.shape[0])
    dt, dev = P.dtype, P.device
    if horiz:
        fp, fq, zp, zq = face[:, :, :-1], face[:, :, 1:], zbuf[:, :, :-1], zbuf[:, :, 1:]
    else:
        fp, fq, zp, zq = face[:, :-1], face[:, 1:], zbuf[:, :-1], zbuf[:, 1:]
    hp, wp = fp.shape[1], fp.shape[2]
    true, false = torch.ones_like(fp, dtype=torch.bool), torch.zeros_like(fp, dtype=torch.bool)
    a_is_p = torch.where(fp < 0, false, torch.where(fq < 0, true, ~(zq > zp)))
    F = torch.where(a_is_p, fp, fq).long()
    ok = (fp != fq) & (F >= 0) & (F < nf)
    Fc = torch.where(ok, F, torch.zeros_like(F))
    corner = tri[Fc]                                                             # [B, hp, wp, 3]
    ok = ok & ((corner >= 0) & (corner < nv)).all(-1)
    corner = torch.where(ok.unsqueeze(-1), corner, torch.zeros_like(corner))
    bidx = torch.arange(b, device=dev).view(b, 1, 1, 1).expand_as(corner)
    XY = P[bidx, corner]                                                         # [B, hp, wp, 3, 2]
    py = torch.arange(hp, device=dev, dtype=dt).view(1, hp, 1).expand(b, hp, wp)
    px = torch.arange(wp, device=dev, dtype=dt).view(1, 1, wp).expand(b, hp, wp)
    step = (~a_is_p).to(dt)
    ac_u, ac_s = (px + step, py) if horiz else (py + step, px)
    U = XY[..., 0] if horiz else XY[..., 1]
    S = (XY[..., 1] if horiz else XY[..., 0]) - ac_s.unsqueeze(-1)
    zero = torch.zeros_like(ac_u)
    res = {"hit": false, "k": torch.zeros_like(F), "d": zero, "t": zero, "den": zero + 1, "du": zero, "si": zero, "sj": zero}
    for k in range(3):
        i, j, own = k, (k + 1) % 3, (k + 2) % 3
        si, sj = S[..., i], S[..., j]
        cross = (si < 0) != (sj < 0)
        den = torch.where(cross, si - sj, zero + 1)
        t = _div(si, den)
        du = U[..., j] - U[..., i]
        c = U[..., i] + du * t
        d = torch.where(a_is_p, c - ac_u, ac_u - c)
        o = opp[Fc, k].long()
        o_ok = (o >= 0) & (o < nv)
        Po = P[bidx[..., 0], torch.where(o_ok, o, torch.zeros_like(o))]
        ex, ey = XY[..., j, 0] - XY[..., i, 0], XY[..., j, 1] - XY[..., i, 1]
        c_own = ex * (XY[..., own, 1] - XY[..., i, 1]) - ey * (XY[..., own, 0] - XY[..., i, 0])
        c_opp = ex * (Po[..., 1] - XY[..., i, 1]) - ey * (Po[..., 0] - XY[..., i, 0])
        opposite = ((c_own > 0) & (c_opp < 0)) | ((c_own < 0) & (c_opp > 0))
        sil = (o == -1) | (o_ok & ~opposite)
        take = ok & cross & (d >= 0) & (d <= 1) & sil & ~res["hit"]
        res["hit"] = res["hit"] | take
        res["k"] = torch.where(take, torch.full_like(F, k), res["k"])
        for name, val in (("d", d), ("t", t), ("den", den), ("du", du), ("si", si), ("sj", sj)):
            res[name] = torch.where(take, val, res[name])
    past = res["d"] >= 0.5
    res["w"] = torch.where(past, res["d"] - 0.5, 0.5 - res["d"])
    res["recv_is_q"] = past == a_is_p
    res["a_is_p"], res["F"], res["XY"] = a_is_p, F, XY
    return res


def _full(x, horiz, me_is_q, fill):
    """A pair-grid tensor on the pixel grid: at every pixel the value of the pair in which it is q (me_is_q) or p."""
    dim = 2 if horiz else 1
    shape = list(x.shape)
    shape[dim] = 1
    edge = torch.full(shape, fill, dtype=x.dtype, device=x.device)
    return torch.cat((edge, x) if me_is_q else (x, edge), dim)


def _cross(P, tri, opp, face, zbuf):
    """Per direction left, right, upper, lower: (this pixel receives [B, H, W], the neighbour receives, w, shift), with
    neighbour = roll(., shift[0], shift[1] + 2) of a [B, C, H, W] tensor."""
    out = []
    for horiz in (True, False):
        r = analyse(P, tri, opp, face, zbuf, horiz)
        for me_is_q in (True, False):
            recv_me = r["hit"] & (r["recv_is_q"] == me_is_q)
            recv_nb = r["hit"] & (r["recv_is_q"] != me_is_q)
            out.append((_full(recv_me, horiz, me_is_q, False), _full(recv_nb, horiz, me_is_q, False),
                        _full(r["w"], horiz, me_is_q, 0.0), (1 if me_is_q else -1, 1 if horiz else 0)))
    return out


def _forward(image, P, tri, opp, face, zbuf):
    out = image
    for recv_me, _, w, (shift, axis) in _cross(P, tri, opp, face, zbuf):
        nb = torch.roll(image, shift, axis + 2)
        out = torch.where(recv_me.unsqueeze(1), out + w.unsqueeze(1) * (nb - image), out)
    return out


def _backward_image(g, P, tri, opp, face, zbuf):
    gi = g
    for recv_me, recv_nb, w, (shift, axis) in _cross(P, tri, opp, face, zbuf):
        w = w.unsqueeze(1)
        gi = torch.where(recv_me.unsqueeze(1), gi - w * g,
                         torch.where(recv_nb.unsqueeze(1), gi + w * torch.roll(g, shift, axis + 2), gi))
    return gi


def _box(XY, h, w):
    """(x0, y0, x1, y1 int64, finite bool) of corner coordinates XY [..., 3, 2]: the face's box as the kernel takes it
    (x1 < x0 or y1 < y0: empty)."""
    X, Y = XY[..., 0], XY[..., 1]
    finite = torch.isfinite(XY).all(-1).all(-1)
    safe = lambda t: torch.where(finite, t, torch.zeros_like(t)).long()                              # noqa: E731
    x0 = safe((torch.floor(X.min(-1)[0]) - 1.0).clamp(max=float(w)).clamp(min=0.0))
    y0 = safe((torch.floor(Y.min(-1)[0]) - 1.0).clamp(max=float(h)).clamp(min=0.0))
    x1 = safe((torch.ceil(X.max(-1)[0]) + 1.0).clamp(min=-1.0).clamp(max=float(w - 1)))
    y1 = safe((torch.ceil(Y.max(-1)[0]) + 1.0).clamp(min=-1.0).clamp(max=float(h - 1)))
    return x0, y0, x1, y1, finite


def box_pixels(v, tri, size):
    """int64 [B, nf]: how many pixels sr_edge_aa_bwd_corner scans for every face (more than BIG: the face's wave)."""
    h, w = _hw(size)
    x0, y0, x1, y1, finite = _box(pixel_coordinates(v, (h, w))[:, tri], h, w)
    return torch.where(finite, (x1 - x0 + 1).clamp(min=0) * (y1 - y0 + 1).clamp(min=0), torch.zeros_like(x0))


def corner_terms(g, image, P, tri, opp, face, zbuf):
    """The terms that gc sums: (b, F, k, lane, order: int64 [n]; values [n, 4] = (gx_i, gy_i, gx_j, gy_j)) over the pairs
    with an edge that lie in their face's box, horizontal pairs first.  `lane` and `order` give the place of a term in its
    face's sum: the lanes are summed one by one in ascending `order`, then by the tree."""
    b, c, h, w = image.shape
    dt = image.dtype
    hw, nhh = w / 2, -(h / 2)
    parts = []
    for horiz in (True, False):
        r = analyse(P, tri, opp, face, zbuf, horiz)
        hit = r["hit"]
        if horiz:
            ip, iq, gp, gq = image[..., :-1], image[..., 1:], g[..., :-1], g[..., 1:]
        else:
            ip, iq, gp, gq = image[:, :, :-1], image[:, :, 1:], g[:, :, :-1], g[:, :, 1:]
        g_r = torch.where(r["recv_is_q"].unsqueeze(1), gq, gp)
        diff = torch.where(r["a_is_p"].unsqueeze(1), ip - iq, iq - ip)
        gd = torch.zeros_like(r["d"])
        for ch in range(c):
            gd = gd + g_r[:, ch] * diff[:, ch]
        gsd = torch.where(r["a_is_p"], gd, -gd)
        gui, guj = gsd * (1 - r["t"]), gsd * r["t"]
        q = _div(gsd * r["du"], r["den"] * r["den"])
        gsi, gsj = -(q * r["sj"]), q * r["si"]
        gX_i, gY_i, gX_j, gY_j = (gui, gsi, guj, gsj) if horiz else (gsi, gui, gsj, guj)
        vals = torch.stack((gX_i * hw, gY_i * nhh, gX_j * hw, gY_j * nhh), -1)
        x0, y0, x1, y1, finite = _box(r["XY"], h, w)
        idx = hit.nonzero(as_tuple=True)
        bi, py, px = idx
        x0, y0, x1, y1 = x0[idx], y0[idx], x1[idx], y1[idx]
        bw = x1 - x0 + 1
        inside = finite[idx] & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
        n = (py - y0) * bw + (px - x0)
        big = bw * (y1 - y0 + 1) > BIG
        lane = torch.where(big, n % WAVE, torch.zeros_like(n))
        order = 2 * n + (0 if horiz else 1)
        keep = inside.nonzero(as_tuple=True)[0]
        parts.append((bi[keep], r["F"][idx][keep], r["k"][idx][keep], lane[keep], order[keep], vals[idx][keep]))
    return tuple(torch.cat([p[i] for p in parts]) for i in range(6))


def _backward_corners(g, image, P, tri, opp, face, zbuf):
    """gc [B, 3 nf, 3]: the ordered sums of `corner_terms`."""
    b, nf = int(image.shape[0]), int(tri.shape[0])
    bi, F, k, lane, order, vals = corner_terms(g, image, P, tri, opp, face, zbuf)
    gc = vals.new_zeros((b * nf, 3, 3))
    n = int(bi.shape[0])
    if n == 0:
        return gc.view(b, 3 * nf, 3)
    rows = torch.arange(n, device=vals.device)
    six = vals.new_zeros((n, 3, 2))
    six = six.index_put((rows, k), vals[:, 0:2]).index_put((rows, (k + 1) % 3), vals[:, 2:4])
    faces, slot = torch.unique(bi * nf + F, return_inverse=True)
    key = slot * WAVE + lane
    by = torch.sort(key * (int(order.max()) + 1) + order)[1]
    key, six = key[by], six[by].reshape(n, 6)
    first = torch.ones(n, dtype=torch.bool, device=key.device)
    first[1:] = key[1:] != key[:-1]
    start = torch.cummax(torch.where(first, rows, torch.zeros_like(rows)), 0)[0]
    rank = rows - start
    acc = vals.new_zeros((int(faces.shape[0]) * WAVE, 6))
    for r in range(int(rank.max()) + 1):
        sel = (rank == r).nonzero(as_tuple=True)[0]
        acc = acc.index_add(0, key[sel], six[sel])                               # one term per key and pass
    acc = acc.view(-1, WAVE, 6)
    off = WAVE // 2
    while off:
        acc = acc[:, :off] + acc[:, off:2 * off]
        off //= 2
    xy = torch.cat((acc.view(-1, 3, 2), vals.new_zeros((int(faces.shape[0]), 3, 1))), 2)
    return gc.index_put((faces,), xy).view(b, 3 * nf, 3)


def _corners_to_vertices(gc, tri, nv):
    """gv [B, nv, 3] of gc [B, 3 nf, 3]: texture.explode's adjoint."""
    from .rasterize import incidence

    b, nf = int(gc.shape[0]), int(tri.shape[0])
    off, adj = incidence(tri, nv)[:2]
    if native_ok(gc):
        gcc = gc.contiguous()
        gv = torch.empty((b, nv, 3), dtype=gc.dtype, device=gc.device)
        native(gcc).sr_explode_bwd(gv, gcc, off, adj, b, nv, nf)
        return gv
    terms = gc.reshape(b, nf, 3, 3).permute(0, 3, 2, 1).reshape(b * 3, 3 * nf)
    return _ordered_sum(terms, off, adj, nv).view(b, 3, nv).permute(0, 2, 1).contiguous()


class _AntialiasComposite(torch.autograd.Function):
    """The definition as an autograd node: its backward is the stated formulas in torch operations, the ordered sums
    included (not what autograd would derive from the forward, which rounds and orders differently)."""

    @staticmethod
    def forward(ctx, image, v, tri, opp, face, zbuf):
        ctx.save_for_backward(image, v, tri, opp, face, zbuf)
        return _forward(image, pixel_coordinates(v, image.shape[2:]), tri, opp, face, zbuf)

    @staticmethod
    def backward(ctx, g):
        image, v, tri, opp, face, zbuf = ctx.saved_tensors
        P = pixel_coordinates(v, image.shape[2:])
        gi = gv = None
        if ctx.needs_input_grad[0]:
            gi = _backward_image(g, P, tri, opp, face, zbuf)
        if ctx.needs_input_grad[1]:
            gv = _corners_to_vertices(_backward_corners(g, image, P, tri, opp, face, zbuf), tri, int(v.shape[1]))
        return gi, gv, None, None, None, None


def _check(image, v, tri, face, zbuf, opp):
    if image.dim() != 4 or not image.is_floating_point():
        raise ValueError("antialias: image must be a floating-point [B, C, H, W], got %s %s"
                         % (image.dtype, tuple(image.shape)))
    b, _, h, w = image.shape
    if v.dim() != 3 or v.shape[0] != b or v.shape[2] != 3 or v.dtype != image.dtype or v.device != image.device:
        raise ValueError("antialias: v must be [%d, nv, 3] of image's float type and device, got %s %s"
                         % (b, v.dtype, tuple(v.shape)))
    if tri.dim() != 2 or tri.shape[1] != 3 or tri.dtype != torch.int64 or tri.device != v.device:
        raise ValueError("antialias: tri must be int64 [nf, 3] on v's device (the adjacency is cached per topology tensor)")
    if face.dtype != torch.int32 or tuple(face.shape) != (b, h, w) or face.device != v.device:
        raise ValueError("antialias: face must be int32 [%d, %d, %d] on v's device, got %s %s"
                         % (b, h, w, face.dtype, tuple(face.shape)))
    if zbuf.dtype != v.dtype or tuple(zbuf.shape) != (b, h, w) or zbuf.device != v.device:
        raise ValueError("antialias: zbuf must be [%d, %d, %d] of v's float type and device, got %s %s"
                         % (b, h, w, zbuf.dtype, tuple(zbuf.shape)))
    if opp.dtype != torch.int32 or tuple(opp.shape) != tuple(tri.shape) or opp.device != v.device:
        raise ValueError("antialias: opp must be int32 %s on v's device (adjacency), got %s %s"
                         % (tuple(tri.shape), opp.dtype, tuple(opp.shape)))


def antialias_composite(image, v, tri, face=None, zbuf=None, opp=None):
    """The defining tensor algebra of `antialias`, in image's float type."""
    face, zbuf, opp = _defaults(image, v, tri, face, zbuf, opp)
    _check(image, v, tri, face, zbuf, opp)
    if image.numel() == 0 or tri.shape[0] == 0 or v.shape[1] == 0:
        return image + torch.zeros_like(image)
    return _AntialiasComposite.apply(image, v, tri, opp, face, zbuf)


# ---- the kernels -------------------------------------------------------------------------------------------------------
def native_ok(*tensors):
    return all(is_device_tensor(t) and t.dtype == torch.float32 for t in tensors if t is not None)


def _dims(image, v, tri):
    b, c, h, w = (int(x) for x in image.shape)
    return b, c, h, w, int(v.shape[1]), int(tri.shape[0])


class _AntialiasNative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, v, tri, opp, face, zbuf):
        ic, vc, tc, oc, fc, zc = (t.contiguous() for t in (image, v, tri, opp, face, zbuf))
        out = torch.empty_like(ic)
        native(ic).sr_edge_aa_fwd(out, ic, vc, tc, oc, fc, zc, *_dims(ic, vc, tc))
        ctx.save_for_backward(ic, vc, tc, oc, fc, zc)
        ctx.tri = tri                                    # the tensor the incidence list is cached by
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ic, vc, tc, oc, fc, zc = ctx.saved_tensors
        g = g.contiguous()
        dims = _dims(ic, vc, tc)
        run = native(ic)
        gi = gv = None
        if ctx.needs_input_grad[0]:
            gi = torch.empty_like(ic)
            run.sr_edge_aa_bwd_image(gi, g, vc, tc, oc, fc, zc, *dims)
        if ctx.needs_input_grad[1]:
            gc = torch.empty((dims[0], 3 * dims[5], 3), dtype=ic.dtype, device=ic.device)
            run.sr_edge_aa_bwd_corner(gc, g, ic, vc, tc, oc, fc, zc, *dims)
            gv = _corners_to_vertices(gc, ctx.tri, dims[4])
        return gi, gv, None, None, None, None


def _defaults(image, v, tri, face, zbuf, opp):
    if (face is None) != (zbuf is None):
        raise ValueError("antialias: face and zbuf come together (face_map), or neither")
    if face is None:
        face, zbuf = face_map(v, tri, tuple(image.shape[2:]))
    if opp is None:
        opp = adjacency(tri, int(v.shape[1]))
    return face, zbuf, opp


def antialias(image, v, tri, face=None, zbuf=None, opp=None):
    """out [B, C, H, W]: image [B, C, H, W] with the pixels on either side of every silhouette edge of the posed mesh v
    [B, nv, 3], tri int64 [nf, 3] blended by where the edge lies between their centres (the module's note).  face, zbuf:
    `face_map(v, tri, (H, W))` (taken when not given); opp: `adjacency(tri, nv)`.  Differentiable in image and in the x and y
    of v; z gets exactly 0.  Device float32 runs sr_edge_aa_fwd and, backward, sr_edge_aa_bwd_image, sr_edge_aa_bwd_corner
    and sr_explode_bwd; everything else `antialias_composite`."""
    face, zbuf, opp = _defaults(image, v, tri, face, zbuf, opp)
    _check(image, v, tri, face, zbuf, opp)
    if image.numel() == 0 or tri.shape[0] == 0 or v.shape[1] == 0:
        return antialias_composite(image, v, tri, face, zbuf, opp)
    if not native_ok(image, v, zbuf):
        if is_device_tensor(image) and strict_native():
            raise RuntimeError("antialias: SR_STRICT_NATIVE=1 and the kernels take float32 device tensors only")
        return antialias_composite(image, v, tri, face, zbuf, opp)
    return _AntialiasNative.apply(image, v, tri, opp, face, zbuf)


def coverage(v, tri, size, face=None, zbuf=None, opp=None):
    """alpha [B, H, W]: `antialias` of the hard cover (1 where a face is drawn, 0 elsewhere) of the posed mesh v [B, nv, 3],
    tri int64 [nf, 3] at size = S or (H, W).  Differentiable in the x and y of v."""
    h, w = _hw(size)
    if face is None:
        face, zbuf = face_map(v, tri, (h, w))
    hard = (face >= 0).to(v.dtype).unsqueeze(1)
    return antialias(hard, v, tri, face, zbuf, opp)[:, 0]
